// knobs.h — the one table of the process-wide test / measurement switches (common.h: test_knobs_armed).
//
// A knob is declared once, beside the code it steers:
//     static int& g_direct = knob("conv_direct", "MRCNN_DIRECT", 3);
// `key` is what mrcnn_debug_set takes, `env` the environment override of the default (nullptr: the knob has none), honoured like
// every override only in a process started with MRCNN_TEST_KNOBS=1 (knob_env).  An override that is unset OR EMPTY leaves the default.
// The returned reference is the knob's storage for the life of the process: reading it is an int load.
//
// The table is a function-local static, so the declarations — initialisers of statics in whatever translation unit — may run in any order.
#pragma once
#include <deque>
#include <map>
#include <string>

#include "common.h"

namespace mrcnn {

struct KnobTable {
    std::deque<int> values;                       // (a deque never moves its elements)
    std::multimap<std::string, int*> by_key;      // one key may set several values ("conv_min_blocks")
};
inline KnobTable& knob_table()
{
    static KnobTable t;
    return t;
}

// also_key: a second key that sets this knob too, along with whatever else carries it
inline int& knob(const char* key, const char* env, int dflt, const char* also_key = nullptr)
{
    KnobTable& t = knob_table();
    const char* e = env ? knob_env(env) : nullptr;
    t.values.push_back(e && *e ? atoi(e) : dflt);
    int* v = &t.values.back();
    t.by_key.emplace(key, v);
    if (also_key) t.by_key.emplace(also_key, v);
    return *v;
}

// false = no knob has that key
inline bool knob_set(const char* key, int value)
{
    const auto range = knob_table().by_key.equal_range(key);
    for (auto it = range.first; it != range.second; ++it) *it->second = value;
    return range.first != range.second;
}

}  // namespace mrcnn

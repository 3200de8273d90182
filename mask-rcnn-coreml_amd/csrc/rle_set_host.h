// rle_set_host.h — the flat RLE set every run-length mask entry takes, its host rule written once: the checks that need neither counts
// nor run_offsets, the checks of run_offsets, of the sums, and the answers the device entries give in the same words.  Plain C++17: no
// HIP header, builds with g++ alone.  A check returns a status and writes its message, which begins with the entry's name, into *err.
#pragma once
#include <string>

#include "ragged.h"

namespace mrcnn {
namespace rle_set {

// A flat RLE set: RLE k is counts[run_offsets[k] .. run_offsets[k+1]) and encodes a heights[k] x widths[k] plane, column-major.
// heights and widths are host arrays of n; counts and run_offsets may be device memory.
struct Flat {
    const uint32_t* counts; const int64_t* run_offsets; int64_t n;
    const int32_t* heights; const int32_t* widths;
};

// What can be answered without reading counts or run_offsets.  check_flat is its two halves in turn; an entry with arguments of its own
// that were judged between them keeps its order by calling the halves.
//   check_flat_pointers: n < 0 -> MRCNN_ERR_SHAPE; null run_offsets, null heights or widths with n > 0 -> MRCNN_ERR_INVALID
//   check_flat_sides:    2^31 RLEs or more, a side outside 1..32767 -> MRCNN_ERR_SHAPE (the message names the RLE)
int check_flat_pointers(const Flat& s, const char* who, std::string* err);
int check_flat_sides(const Flat& s, const char* who, std::string* err);
int check_flat(const Flat& s, const char* who, std::string* err);

// run_offsets (host memory, n + 1 entries): non-negative and not decreasing (MRCNN_ERR_SHAPE naming the RLE)
int check_run_offsets(const int64_t* run_offsets, int64_t n, const char* who, std::string* err);
// counts may be null exactly when the set has no runs (MRCNN_ERR_INVALID); run_offsets has passed check_run_offsets
int check_counts(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const char* who, std::string* err);
// an RLE set in host memory: check_run_offsets, check_counts, then every RLE sums to its plane (the lowest k that does not is named)
int check_sums(const Flat& s, const char* who, std::string* err);

// the answer to an RLE that does not sum to its plane, shared with the device entries, which find the RLE on the device
int bad_sum(const Flat& s, int64_t k, unsigned long long sum, const char* who, std::string* err);
// the answer to a capacity below the runs of the result
int bad_runs_capacity(long long need, long long capacity, const char* who, std::string* err);

}  // namespace rle_set
}  // namespace mrcnn

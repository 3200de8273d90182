// rle_set_host.cpp — see rle_set_host.h.
#include "rle_set_host.h"

namespace mrcnn {
namespace rle_set {

int check_flat_pointers(const Flat& s, const char* who, std::string* err)
{
    if (s.n < 0) return bad(err, MRCNN_ERR_SHAPE, "%s: n %lld is negative", who, (long long)s.n);
    if (!s.run_offsets || ((!s.heights || !s.widths) && s.n > 0)) return bad(err, MRCNN_ERR_INVALID, "%s: null argument", who);
    return MRCNN_OK;
}

int check_flat_sides(const Flat& s, const char* who, std::string* err)
{
    if (s.n >= (1LL << 31)) return bad(err, MRCNN_ERR_SHAPE, "%s: %lld RLEs are too many", who, (long long)s.n);
    for (int64_t k = 0; k < s.n; ++k)
        if (s.heights[k] < 1 || s.heights[k] > 32767 || s.widths[k] < 1 || s.widths[k] > 32767)
            return bad(err, MRCNN_ERR_SHAPE, "%s: RLE %lld is %dx%d: height and width must lie in 1..32767", who, (long long)k, s.heights[k], s.widths[k]);
    return MRCNN_OK;
}

int check_flat(const Flat& s, const char* who, std::string* err)
{
    const int st = check_flat_pointers(s, who, err);
    return st != MRCNN_OK ? st : check_flat_sides(s, who, err);
}

int check_run_offsets(const int64_t* run_offsets, int64_t n, const char* who, std::string* err)
{
    if (run_offsets[0] < 0) return bad(err, MRCNN_ERR_SHAPE, "%s: run_offsets[0] = %lld is negative", who, (long long)run_offsets[0]);
    for (int64_t k = 0; k < n; ++k)
        if (run_offsets[k + 1] < run_offsets[k]) return bad(err, MRCNN_ERR_SHAPE, "%s: run_offsets decrease at RLE %lld", who, (long long)k);
    return MRCNN_OK;
}

int check_counts(const uint32_t* counts, const int64_t* run_offsets, int64_t n, const char* who, std::string* err)
{
    if (!counts && run_offsets[n] > run_offsets[0]) return bad(err, MRCNN_ERR_INVALID, "%s: null counts", who);
    return MRCNN_OK;
}

int check_sums(const Flat& s, const char* who, std::string* err)
{
    int st = check_run_offsets(s.run_offsets, s.n, who, err);
    if (st == MRCNN_OK) st = check_counts(s.counts, s.run_offsets, s.n, who, err);
    if (st != MRCNN_OK) return st;
    for (int64_t k = 0; k < s.n; ++k) {
        uint64_t sum = 0;
        for (int64_t j = s.run_offsets[k]; j < s.run_offsets[k + 1]; ++j) sum += s.counts[j];
        if (sum != (uint64_t)s.heights[k] * (uint64_t)s.widths[k]) return bad_sum(s, k, sum, who, err);
    }
    return MRCNN_OK;
}

int bad_sum(const Flat& s, int64_t k, unsigned long long sum, const char* who, std::string* err)
{
    return bad(err, MRCNN_ERR_SHAPE, "%s: RLE %lld sums to %llu pixels, its %dx%d plane has %llu", who, (long long)k, sum, s.heights[k], s.widths[k],
               (unsigned long long)s.heights[k] * (unsigned long long)s.widths[k]);
}

int bad_runs_capacity(long long need, long long capacity, const char* who, std::string* err)
{
    return bad(err, MRCNN_ERR_SHAPE, "%s: the set encodes to %lld runs, out_counts holds %lld: call again with capacity >= %lld", who, need, capacity, need);
}

}  // namespace rle_set
}  // namespace mrcnn

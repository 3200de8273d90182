// kernels_coco_acc.hip — COCOeval.accumulate on the device (mrcnn_coco_accumulate): a segmented stable sort of the detection entries
// by descending score, then the tp / fp prefix counts, the precision envelope and the recall-threshold lookup per (category, area
// range, maxDets, IoU threshold).  Built with -ffp-contract=off: the only floating-point operations are the two IEEE double divisions
// and the one addition of coco_eval.accumulate, on integers counted exactly, so the results are that function's, bit for bit.
//
// Sort.  Entry i gets one 64-bit key that orders like -score (acc_key); a category (a SEGMENT of the flat list) is cut into chunks of
// COCO_ACC_CHUNK entries counted from the segment's start.  k_acc_sort_chunks sorts every chunk in LDS by (key, position) — a bitonic
// network, made stable by the position — and k_acc_merge then merges neighbouring sorted runs of a segment pairwise, doubling the run
// length per launch: every entry finds its place in the merged run by a binary search of the other run (lower bound from the left run,
// upper bound from the right one, which keeps equal keys in their order).  The launches number 1 + ceil(log2(chunks of the longest
// segment)), whatever the number of categories.
//
// Layout of the flags.  The two (A*T, n_dt) byte planes are permuted ONCE into sorted order and folded into one byte per entry
// (k_acc_permute: 0 = false positive, 1 = true positive, 2 = ignored); the ranks likewise.  The scan kernel, which reads every plane
// once per maxDets value, then reads consecutive bytes instead of gathering through the permutation.
#include "kernels.h"

namespace mrcnn {
namespace {

constexpr int WAVE = 64;
constexpr int ACC_BLOCK = 256;
constexpr int ACC_WAVES = ACC_BLOCK / WAVE;
constexpr int ACC_ITEMS = COCO_ACC_CHUNK / ACC_BLOCK;       // consecutive entries per thread and chunk in the scan
static_assert(COCO_ACC_CHUNK == ACC_BLOCK * ACC_ITEMS && (COCO_ACC_CHUNK & (COCO_ACC_CHUNK - 1)) == 0, "the chunk is a power of two and a multiple of the block");
typedef unsigned long long u64;

// ascending key <=> np.argsort(-score): -0 and 0 are one key, a NaN is the largest key of all
__device__ __forceinline__ u64 acc_key(double score)
{
    if (score != score) return ~0ULL;
    const double v = score == 0.0 ? 0.0 : -score;
    const long long b = __double_as_longlong(v);
    return b < 0 ? ~(u64)b : ((u64)b | 0x8000000000000000ULL);
}

// One block per chunk: keys from the scores, sorted in LDS by (key, position in the chunk); 12 KiB of LDS.
__global__ __launch_bounds__(ACC_BLOCK) void k_acc_sort_chunks(const double* __restrict__ scores, const AccChunk* __restrict__ chunks,
                                                               u64* __restrict__ keys_out, uint32_t* __restrict__ perm_out)
{
    __shared__ u64 key[COCO_ACC_CHUNK];
    __shared__ uint32_t idx[COCO_ACC_CHUNK];
    const AccChunk C = chunks[blockIdx.x];
    const int cnt = min(COCO_ACC_CHUNK, C.seg_len - C.at);
    const long long g0 = C.seg0 + C.at;
    for (int i = threadIdx.x; i < COCO_ACC_CHUNK; i += ACC_BLOCK) {
        key[i] = i < cnt ? acc_key(scores[g0 + i]) : ~0ULL;      // the padding sorts behind every entry: largest key, larger position
        idx[i] = (uint32_t)i;
    }
    __syncthreads();
    for (int k = 2; k <= COCO_ACC_CHUNK; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < COCO_ACC_CHUNK / 2; t += ACC_BLOCK) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const u64 ki = key[i], kl = key[l];
                const uint32_t ii = idx[i], il = idx[l];
                const bool gt = ki > kl || (ki == kl && ii > il);
                if (gt == ((i & k) == 0)) { key[i] = kl; key[l] = ki; idx[i] = il; idx[l] = ii; }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < cnt; i += ACC_BLOCK) {
        keys_out[g0 + i] = key[i];
        perm_out[g0 + i] = (uint32_t)(g0 + idx[i]);
    }
}

// One block per chunk: the sorted runs of `run` entries of a segment are merged in pairs.  A chunk lies inside one run (run is a multiple
// of the chunk), so the run searched is the same for the whole block.  A run without a partner is copied.
__global__ __launch_bounds__(ACC_BLOCK) void k_acc_merge(const AccChunk* __restrict__ chunks, long long run, const u64* __restrict__ keys_in,
                                                         const uint32_t* __restrict__ perm_in, u64* __restrict__ keys_out, uint32_t* __restrict__ perm_out)
{
    const AccChunk C = chunks[blockIdx.x];
    const long long n = C.seg_len, r = C.at / run;
    const long long pair0 = (r >> 1) * 2 * run, mid = min(pair0 + run, n), end = min(pair0 + 2 * run, n);
    const bool left = (r & 1) == 0;
    const u64* kin = keys_in + C.seg0;
    for (int j = 0; j < ACC_ITEMS; ++j) {
        const long long p = C.at + j * ACC_BLOCK + threadIdx.x;
        if (p >= n) break;
        const u64 key = kin[p];
        long long lo = left ? mid : pair0, hi = left ? end : mid;
        while (lo < hi) {
            const long long m = (lo + hi) >> 1;
            const u64 km = kin[m];
            if (left ? km < key : km <= key) lo = m + 1; else hi = m;
        }
        const long long pos = left ? p + (lo - mid) : (p - mid) + lo;
        keys_out[C.seg0 + pos] = key;
        perm_out[C.seg0 + pos] = perm_in[C.seg0 + p];
    }
}

// code[plane][i] and srank[i] for sorted position i: consecutive writes, gathered reads, once per call
__global__ __launch_bounds__(ACC_BLOCK) void k_acc_permute(const uint32_t* __restrict__ perm, const int32_t* __restrict__ ranks,
                                                           const uint8_t* __restrict__ matched, const uint8_t* __restrict__ ignore, long long n_dt,
                                                           int planes, uint8_t* __restrict__ code, int32_t* __restrict__ srank)
{
    const long long i = (long long)blockIdx.x * ACC_BLOCK + threadIdx.x;
    if (i >= n_dt) return;
    const long long src = perm[i];
    if (blockIdx.y == 0) srank[i] = ranks[src];
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const long long o = (long long)pl * n_dt;
        code[o + i] = ignore[o + src] ? 2 : (matched[o + src] ? 1 : 0);
    }
}

__device__ __forceinline__ u64 acc_flag(int code) { return code == 1 ? 1ULL << 32 : (code == 0 ? 1ULL : 0ULL); }      // tp in the high word, fp in the low

// inclusive sum over the block; `sh` holds ACC_WAVES entries and is free again on return
__device__ __forceinline__ u64 acc_block_scan(u64 v, u64* sh, u64& total)
{
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const u64 t = __shfl_up(v, d, WAVE);
        if (lane >= d) v += t;
    }
    if (lane == WAVE - 1) sh[wave] = v;
    __syncthreads();
    u64 add = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < ACC_WAVES; ++w) { const u64 x = sh[w]; if (w < wave) add += x; tot += x; }
    __syncthreads();
    total = tot;
    return v + add;
}

// the number of thresholds <= x (thr is non-decreasing)
__device__ __forceinline__ int acc_count_le(const double* __restrict__ thr, int R, double x)
{
    int lo = 0, hi = R;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (thr[m] <= x) lo = m + 1; else hi = m;
    }
    return lo;
}

// One block per (category k, area range a, maxDets m, threshold t).  An entry TAKES PART when its rank is below maxDets.
//   forward:  the tp / fp / taking-part totals of the segment (integers).
//   backward: chunk by chunk from the end.  The prefix counts at a chunk's start are the counts at its end minus the chunk's own — exact,
//             they are integers — so no prefix has to be stored.  Per entry pr = tp / ((fp + tp) + eps); the envelope is the running maximum
//             from the end, carried from chunk to chunk; the entry at which tp steps from c - 1 to c is the first with rc >= thr for exactly
//             the thresholds in ((c - 1) / npig, c / npig], and writes the envelope there.  Thresholds <= 0 are met by the first entry that
//             takes part, whose envelope is the maximum over all; thresholds above the last rc stay 0.
__global__ __launch_bounds__(ACC_BLOCK) void k_acc_scan(const uint8_t* __restrict__ code, const int32_t* __restrict__ srank,
                                                        const long long* __restrict__ cat_off, const long long* __restrict__ npig,
                                                        const int32_t* __restrict__ max_dets, const double* __restrict__ thr, long long n_dt, int K,
                                                        int A, int M, int T, int R, double* __restrict__ precision, double* __restrict__ recall)
{
    __shared__ u64 sh[ACC_WAVES];
    __shared__ uint32_t sh_n[ACC_WAVES];
    __shared__ double sh_m[ACC_WAVES];
    const long long b = blockIdx.x;
    const int t = (int)(b % T), m = (int)(b / T % M), a = (int)(b / ((long long)T * M) % A), k = (int)(b / ((long long)T * M * A));
    const long long seg0 = cat_off[k], n = cat_off[k + 1] - seg0, np = npig[(long long)k * A + a];
    const long long p_stride = (long long)K * A * M;                                   // between two recall thresholds of `precision`
    double* const q = precision + (long long)t * R * p_stride + ((long long)k * A + a) * M + m;
    double* const rec = recall + (((long long)t * K + k) * A + a) * M + m;
    if (np == 0) {
        for (int r = threadIdx.x; r < R; r += ACC_BLOCK) q[r * p_stride] = -1.0;
        if (threadIdx.x == 0) *rec = -1.0;
        return;
    }
    const int md = max_dets[m];
    const uint8_t* const cd = code + ((long long)a * T + t) * n_dt + seg0;
    const int32_t* const rk = srank + seg0;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;

    u64 mine = 0;
    uint32_t mine_n = 0;
    for (long long p = threadIdx.x; p < n; p += ACC_BLOCK)
        if (rk[p] < md) { mine += acc_flag(cd[p]); ++mine_n; }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) { mine += __shfl_xor(mine, o, WAVE); mine_n += __shfl_xor(mine_n, o, WAVE); }
    if (lane == 0) { sh[wave] = mine; sh_n[wave] = mine_n; }
    __syncthreads();
    u64 end = 0;
    uint32_t nd = 0;
#pragma unroll
    for (int w = 0; w < ACC_WAVES; ++w) { end += sh[w]; nd += sh_n[w]; }
    __syncthreads();
    const double dnp = (double)np, rc_last = (double)(end >> 32) / dnp;
    const int r_end = nd ? acc_count_le(thr, R, rc_last) : 0;                          // thresholds from here on are never reached

    double carry = -1.0;                                                               // (every pr is >= 0)
    for (long long c = (n + COCO_ACC_CHUNK - 1) / COCO_ACC_CHUNK - 1; c >= 0; --c) {
        const long long base = c * COCO_ACC_CHUNK + (long long)threadIdx.x * ACC_ITEMS;
        u64 f[ACC_ITEMS], s = 0;
        bool part[ACC_ITEMS];
#pragma unroll
        for (int i = 0; i < ACC_ITEMS; ++i) {
            const long long p = base + i;
            part[i] = p < n && rk[p] < md;
            f[i] = part[i] ? acc_flag(cd[p]) : 0ULL;
            s += f[i];
        }
        u64 chunk;
        const u64 incl = acc_block_scan(s, sh, chunk);
        const u64 start = end - chunk;                                                 // both words at once: neither borrows
        u64 at = start + incl - s;
        double pr[ACC_ITEMS];
        uint32_t tp[ACC_ITEMS];
#pragma unroll
        for (int i = 0; i < ACC_ITEMS; ++i) {
            at += f[i];
            tp[i] = (uint32_t)(at >> 32);
            const double dtp = (double)tp[i], dfp = (double)(uint32_t)at;
            pr[i] = part[i] ? dtp / ((dfp + dtp) + 2.220446049250313e-16) : -1.0;
        }
        double env[ACC_ITEMS];
        env[ACC_ITEMS - 1] = pr[ACC_ITEMS - 1];
#pragma unroll
        for (int i = ACC_ITEMS - 2; i >= 0; --i) env[i] = fmax(pr[i], env[i + 1]);
        double v = env[0];                                                             // the maximum from this thread's entries to the wave's end
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const double o = __shfl_down(v, d, WAVE);
            if (lane + d < WAVE) v = fmax(v, o);
        }
        double after = __shfl_down(v, 1, WAVE);
        if (lane == WAVE - 1) after = -1.0;
        if (lane == 0) sh_m[wave] = v;
        __syncthreads();
        double all = carry;
        after = fmax(after, carry);
#pragma unroll
        for (int w = 0; w < ACC_WAVES; ++w) { const double x = sh_m[w]; if (w > wave) after = fmax(after, x); all = fmax(all, x); }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ACC_ITEMS; ++i) {
            if (!(f[i] >> 32)) continue;                                               // only a true positive moves rc
            const double e = fmax(env[i], after);
            const int r0 = acc_count_le(thr, R, (double)(tp[i] - 1) / dnp), r1 = acc_count_le(thr, R, (double)tp[i] / dnp);
            for (int r = r0; r < r1; ++r) q[r * p_stride] = e;
        }
        carry = all;
        end = start;
    }
    const int r_zero = nd ? acc_count_le(thr, R, 0.0) : 0;
    for (int r = threadIdx.x; r < r_zero; r += ACC_BLOCK) q[r * p_stride] = carry;
    for (int r = r_end + threadIdx.x; r < R; r += ACC_BLOCK) q[r * p_stride] = 0.0;
    if (threadIdx.x == 0) *rec = nd ? rc_last : 0.0;
}

}  // namespace

const uint32_t* coco_acc_sort_forward(hipStream_t s, const double* scores, const AccChunk* chunks, long n_chunks, long long longest, u64* keys_a,
                                      uint32_t* perm_a, u64* keys_b, uint32_t* perm_b)
{
    if (n_chunks <= 0) return perm_a;
    hipLaunchKernelGGL(k_acc_sort_chunks, dim3((unsigned)n_chunks), dim3(ACC_BLOCK), 0, s, scores, chunks, keys_a, perm_a);
    HIP_CHECK(hipGetLastError());
    for (long long run = COCO_ACC_CHUNK; run < longest; run *= 2) {
        hipLaunchKernelGGL(k_acc_merge, dim3((unsigned)n_chunks), dim3(ACC_BLOCK), 0, s, chunks, run, keys_a, perm_a, keys_b, perm_b);
        HIP_CHECK(hipGetLastError());
        std::swap(keys_a, keys_b); std::swap(perm_a, perm_b);
    }
    return perm_a;
}

void coco_acc_permute_forward(hipStream_t s, const uint32_t* perm, const int32_t* ranks, const uint8_t* matched, const uint8_t* ignore, long long n_dt,
                              int planes, uint8_t* code, int32_t* srank)
{
    if (n_dt <= 0) return;
    hipLaunchKernelGGL(k_acc_permute, dim3((unsigned)((n_dt + ACC_BLOCK - 1) / ACC_BLOCK), (unsigned)std::min(planes, 65535)), dim3(ACC_BLOCK), 0, s, perm,
                       ranks, matched, ignore, n_dt, planes, code, srank);
    HIP_CHECK(hipGetLastError());
}

void coco_acc_scan_forward(hipStream_t s, const uint8_t* code, const int32_t* srank, const long long* cat_off, const long long* npig,
                           const int32_t* max_dets, const double* rec_thrs, long long n_dt, int K, int A, int M, int T, int R, double* precision,
                           double* recall)
{
    const long long blocks = (long long)K * A * M * T;
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_acc_scan, dim3((unsigned)blocks), dim3(ACC_BLOCK), 0, s, code, srank, cat_off, npig, max_dets, rec_thrs, n_dt, K, A, M, T, R,
                       precision, recall);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn

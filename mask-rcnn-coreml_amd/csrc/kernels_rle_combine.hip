// kernels_rle_combine.hip — the set algebra of run-length masks (mrcnn_rle_combine): union, intersection, symmetric difference and
// difference of the members of a group, RLE in, RLE out, no dense byte plane and no scratch of an image's size.  The rule is
// combine_rule.h's; rle_combine_host.cpp is the definition.
//
// The result of a group is written as a packed BIT BOX laid out as kernels_rle_morph.hip lays its own out — the box the result lies in,
// 32 rows per uint32 word, word (j, c) of a box of bw columns at j * bw + c — and that file's encoder runs on the bits.
//   k_combine   one thread per column of a group's box.  The thread keeps the words of its column in LDS as [word][thread] — lanes touch
//               consecutive 4-byte words, so no bank is hit twice, and no thread reads another's words, so there is no barrier — and folds
//               the members in their order: for every member whose tight box holds the column, one binary search in the member's prefix
//               table and a walk of the column's runs of ones.  The first member's intervals are set; a later member's are set (OR),
//               toggled (XOR) or cleared (DIFF), and for AND the gaps between them are cleared.  32 words are 1024 rows: a taller box
//               takes several passes, each restarting its walks at the pass's first row with one more search.  Each word row goes to
//               global memory once, coalesced across the block's columns.  A thread owns its column: nothing is atomic.
// One launch whatever the number of RLEs, of groups and of members: a group of 100 members is one loop inside a thread.
#include "kernels.h"
#include "combine_rule.h"
#include "scan_device.h"

namespace mrcnn {
namespace {

enum { COMBINE_SET, COMBINE_TOGGLE, COMBINE_CLEAR };

__global__ __launch_bounds__(256) void k_combine(const CombineJob job)
{
    __shared__ uint32_t lds[COMBINE_PASS_WORDS][256];        // 32 KB: column threadIdx.x is this thread's own
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= job.cols) return;
    const int k = last_not_above(job.n, g, [&](int i) { return job.rec[i].col0; });
    const MorphRec q = job.rec[k];
    const int bw = q.work.x2 - q.work.x1, c = (int)(g - q.col0), x = q.work.x1 + c;
    const long long m0 = job.member0[k], m1 = job.member0[k + 1];
    uint32_t* out = job.bits + q.word0 + c;
    const int t = threadIdx.x;

    for (int j0 = 0; j0 < q.words; j0 += COMBINE_PASS_WORDS) {
        const int nw = min(COMBINE_PASS_WORDS, q.words - j0);
        const int ya = q.work.y1 + 32 * j0, yb = min(q.work.y2, ya + 32 * nw);      // the pass's rows: bit i of the pass is row ya + i
        for (int j = 0; j < nw; ++j) lds[j][t] = 0u;
        auto apply = [&](int kind, int a, int b) {               // bits [a, b) of the pass (held to its words: nothing is touched outside them)
            a = max(a, 0); b = min(b, 32 * nw);
            while (a < b) {
                const int wj = a >> 5, top = min(b, (wj + 1) << 5), n = top - a;
                const uint32_t mask = (n == 32 ? 0xffffffffu : (1u << n) - 1u) << (a & 31);
                const uint32_t v = lds[wj][t];
                lds[wj][t] = kind == COMBINE_SET ? v | mask : (kind == COMBINE_TOGGLE ? v ^ mask : v & ~mask);
                a = top;
            }
        };
        const uint32_t p0 = (uint32_t)x * (uint32_t)q.h + (uint32_t)ya, p1 = p0 + (uint32_t)(yb - ya);
        for (long long m = m0; m < m1; ++m) {
            const CombineMember e = job.members[m];
            const bool first = m == m0;
            const bool gaps = !first && job.op == MRCNN_RLE_AND; // acc & member: what the member leaves unset is cleared
            const int kind = first || job.op == MRCNN_RLE_OR ? COMBINE_SET : (job.op == MRCNN_RLE_XOR ? COMBINE_TOGGLE : COMBINE_CLEAR);
            int done = 0;                                        // AND: the end of the member's last interval
            if (x >= e.tight.x1 && x < e.tight.x2 && ya < e.tight.y2 && yb > e.tight.y1) {      // (else the member has no set pixel here)
                const uint32_t* B = job.pre_b + e.r0;
                const uint32_t* cnt = job.counts + e.r0;
                for (int j = last_not_above(e.nruns, (long long)p0, [&](int i) { return (long long)B[i]; }); j < e.nruns; ++j) {
                    const uint32_t s = B[j];
                    if (s >= p1) break;
                    const uint32_t n = cnt[j];
                    if (!(j & 1) || !n) continue;
                    const int a = (int)(max(s, p0) - p0), b = (int)(min(s + n, p1) - p0);
                    if (gaps) { apply(COMBINE_CLEAR, done, a); done = b; }
                    else apply(kind, a, b);
                }
            }
            if (gaps) apply(COMBINE_CLEAR, done, yb - ya);
        }
        for (int j = 0; j < nw; ++j) out[(long long)(j0 + j) * bw] = lds[j][t];
    }
}

}  // namespace

void rle_combine_forward(hipStream_t s, const CombineJob& job)
{
    if (job.cols <= 0) return;
    hipLaunchKernelGGL(k_combine, dim3((unsigned)((job.cols + 255) / 256)), dim3(256), 0, s, job);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn

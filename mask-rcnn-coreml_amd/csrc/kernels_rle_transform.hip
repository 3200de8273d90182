// kernels_rle_transform.hip — run-length masks moved to another pixel grid (mrcnn_rle_transform): crop, place, flip, transpose, the
// rotations and nearest resizes, RLE in, RLE out, no dense byte plane and no scratch of an image's size.  The rule is transform_rule.h's;
// rle_transform_host.cpp is the definition.
//
// The result of an RLE is written as a packed BIT BOX laid out as kernels_rle_morph.hip lays its own out — the box the result lies in,
// 32 rows per uint32 word, word (j, c) of a box of bw columns at j * bw + c — and that file's encoder runs on the bits.
//   k_transform   one thread per column X of a work box.  The thread keeps the words of its column in LDS as [word][thread] — lanes touch
//                 consecutive 4-byte words, so no bank is hit twice, and no thread reads another's words, so there is no barrier.
//                 32 words are 1024 rows: a taller box takes several passes.  Each word row goes to global memory once, coalesced
//                 across the block's columns.
//     plain record       column X reads the source column sx = u(X): one binary search in the prefix table at the first source row the
//                        pass can see, then a walk of that column's runs of ones.  Each interval [a, b) of source rows becomes its range
//                        of Y by the rule's inverse, clipped to the pass, and those bits are set: a run costs O(1) whatever the scale.
//                        A negative ay yields the ranges in falling order, which setting bits does not mind.
//     transposed record  column X reads the source ROW sy = u(X), and row Y the source column sx = v(Y).  The thread walks the Y of the
//                        pass; for every distinct sx one point query — a binary search at position sx*h + sy — finds the run that holds
//                        the pixel: the LAST of equal prefix entries (zero-length runs lie before it), set iff its index is odd.  The bit
//                        is replicated over the Y range that shares sx.  Neighbouring lanes query neighbouring rows of one source
//                        column, so their searches share cache lines.
// A thread owns its column: nothing is atomic and the result does not depend on the order of execution.  A call may mix both kinds of
// record: the columns of one record are contiguous, so waves diverge only at record borders.  One launch whatever the number of RLEs.
#include "kernels.h"
#include "transform_rule.h"
#include "scan_device.h"

namespace mrcnn {
namespace {

__global__ __launch_bounds__(256) void k_transform(const XfJob job)
{
    __shared__ uint32_t lds[XF_PASS_WORDS][256];             // 32 KB: column threadIdx.x is this thread's own
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= job.cols) return;
    const int k = last_not_above(job.n, g, [&](int i) { return job.rec[i].col0; });
    const MorphRec q = job.rec[k];
    const XfSource e = job.src[k];
    const int bw = q.work.x2 - q.work.x1, c = (int)(g - q.col0), X = q.work.x1 + c;
    uint32_t* out = job.bits + q.word0 + c;
    const int t = threadIdx.x;
    const uint32_t* B = job.pre_b + e.r0;
    const uint32_t* cnt = job.counts + e.r0;
    const long long u = xf_source(e.map.x, X);               // the source column, or the source row of a transposed record
    const bool inside = e.map.transpose ? (u >= e.tight.y1 && u < e.tight.y2) : (u >= e.tight.x1 && u < e.tight.x2);

    for (int j0 = 0; j0 < q.words; j0 += XF_PASS_WORDS) {
        const int nw = min(XF_PASS_WORDS, q.words - j0);
        const int ya = q.work.y1 + 32 * j0, yb = min(q.work.y2, ya + 32 * nw);      // the pass's rows: bit i of the pass is row ya + i
        for (int j = 0; j < nw; ++j) lds[j][t] = 0u;
        auto set = [&](int a, int b) {                           // bits [a, b) of the pass (held to its words: nothing is touched outside them)
            a = max(a, 0); b = min(b, 32 * nw);
            while (a < b) {
                const int wj = a >> 5, top = min(b, (wj + 1) << 5), n = top - a;
                lds[wj][t] |= (n == 32 ? 0xffffffffu : (1u << n) - 1u) << (a & 31);
                a = top;
            }
        };
        if (inside && !e.map.transpose) {
            // the source rows the pass can see, held to the rows that have a set pixel
            const long long va = xf_source(e.map.y, ya), vb = xf_source(e.map.y, yb - 1);
            const long long lo = max(min(va, vb), (long long)e.tight.y1), hi = min(max(va, vb) + 1, (long long)e.tight.y2);
            if (lo < hi) {
                const uint32_t top = (uint32_t)u * (uint32_t)e.h, p0 = top + (uint32_t)lo, p1 = top + (uint32_t)hi;
                for (int j = last_not_above(e.nruns, (long long)p0, [&](int i) { return (long long)B[i]; }); j < e.nruns; ++j) {
                    const uint32_t s = B[j];
                    if (s >= p1) break;
                    const uint32_t n = cnt[j];
                    if (!(j & 1) || !n) continue;
                    const long long a = (long long)max(s, p0) - top, b = (long long)min(s + n, p1) - top;
                    if (a >= b) continue;
                    int y0, y1;
                    xf_preimage_in(e.map.y, a, b, ya, yb, &y0, &y1);
                    set(y0 - ya, y1 - ya);
                }
            }
        } else if (inside) {
            for (int Y = ya; Y < yb;) {
                const long long sx = xf_source(e.map.y, Y);
                int y0, y1;
                xf_preimage_in(e.map.y, sx, sx + 1, ya, yb, &y0, &y1);               // the rows that share sx: Y is one of them
                y1 = max(y1, Y + 1);
                if (sx >= e.tight.x1 && sx < e.tight.x2) {
                    const long long p = sx * e.h + u;
                    const int j = last_not_above(e.nruns, p, [&](int i) { return (long long)B[i]; });
                    if (j & 1) set(Y - ya, y1 - ya);
                }
                Y = y1;
            }
        }
        for (int j = 0; j < nw; ++j) out[(long long)(j0 + j) * bw] = lds[j][t];
    }
}

}  // namespace

void rle_transform_forward(hipStream_t s, const XfJob& job)
{
    if (job.cols <= 0) return;
    hipLaunchKernelGGL(k_transform, dim3((unsigned)((job.cols + 255) / 256)), dim3(256), 0, s, job);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn

// kernels_render.hip — drawing detections on gfx950: the instance-id map and the rendered overlay of a ragged batch of
// mixed-size images, straight from the 28×28 masks (mrcnn_instance_map_source, mrcnn_render_detections_source).
//
// Replaces (reference, Example/Source/DetectionRenderer.swift:13-88): renderMask stretches each mask over its box, fills it in
// one of four colours and strokes the box three pixels wide, row after row in painter's order, through CoreGraphics.  Here a
// pixel is decided ONCE: the lowest drawn row whose pasted plane is set owns it (rows arrive in descending score, so the most
// confident instance wins — the reference's painter's order lets the LAST row cover the others; see maskrcnn_hip.h).
//
// The set decisions are the paste's bits: paste_row / paste_pixel of paste_device.h on the pixel boxes k_unletterbox_boxes
// writes, the same float operations in the same order (-ffp-contract=off).  The rows × h × w planes never exist.
//
//   k_instance_map        2·h·w bytes written per image (int16 per pixel); nothing but boxes and masks (L1 / L2) is read.
//   k_render_detections   3·h·w bytes read + 3·h·w bytes written per image (RGB8 in, RGB8 out), the source read once.
//
// Both: ONE launch for the whole batch, grid (tiles, batch).  An image's output is addressed as one flat byte stream, as
// k_paste_masks_ragged does: a lane owns whole 16-byte aligned chunks of it (one chunk = 8 map pixels; three chunks = 48 bytes
// = 16 RGB pixels, plus the two pixels that straddle the ends when the base is not a multiple of 3 bytes away from a pixel
// start), a block owns a TILE of 256 consecutive lanes' worth.  Per tile the block first culls the image's drawn rows — score
// above min_score, non-empty box, the box grown by the stroke's outer part touching the tile's rows (and columns, when the tile
// lies inside one row) — into an LDS list in ascending row index: 256 rows per pass, one per thread, wave ballot + popcount for
// the position.  Every lane then walks that short list over its pixels; a pixel stops taking part at its first hit, a lane
// leaves the list when all its pixels have one, and only a row whose box covers the pixel pays a bilinear sample.  More than
// 256 rows are culled in further passes over the same registers (lower rows first, so a hit is final).
// visible_areas: winners are counted per listed row in LDS (a lane merges runs of equal winners first), then one vector
// atomic per (block, row) that has any.  Bytes before the first and after the last whole chunk go out one by one from block 0.
#include "kernels.h"
#include "draw_rule.h"
#include "paste_device.h"
#include "scan_device.h"

namespace mrcnn {

constexpr int DRAW_ROWS = 256;              // rows culled per pass = threads of a block
struct DrawList {
    int4 box[DRAW_ROWS];                    // (y1, x1, y2, x2) of the listed rows, ascending row index
    int row[DRAW_ROWS];
    int wave_n[DRAW_ROWS / 64];
};

// draw_rule.h's stroke for a box kept as (y1, x1, y2, x2)
__device__ __forceinline__ bool in_ring(const int4 b, int grow, int shrink, int y, int x) { return in_ring(RleDrawBox{b.x, b.y, b.z, b.w}, grow, shrink, y, x); }

// One cull pass: rows [base, base + 256) of the image against the tile's rectangle (inclusive bounds).  Returns the list length.
// Two barriers inside (one of them compact_256's); the caller puts one more behind its walk before the next pass overwrites the list.
__device__ __forceinline__ int cull_rows(DrawList& L, const int4* __restrict__ bx, const float* __restrict__ det, int rows, int base, float min_score,
                                         int grow, int ty0, int ty1, int tx0, int tx1)
{
    const int i = base + (int)threadIdx.x;
    bool keep = false;
    int4 b = make_int4(0, 0, 0, 0);
    if (i < rows) {
        b = bx[i];
        keep = b.z > b.x && b.w > b.y && det[(size_t)i * 6 + 5] > min_score
            && b.x - grow <= ty1 && b.z + grow > ty0 && b.y - grow <= tx1 && b.w + grow > tx0;
    }
    int n;
    const int pos = compact_256(keep, L.wave_n, &n);
    if (keep) {
        L.box[pos] = b;
        L.row[pos] = i;
    }
    __syncthreads();
    return n;
}

// A lane's NP consecutive pixels from flat index q0 against the list: win[k] = the lowest listed row whose plane is set at
// pixel k, ring[k] = the lowest whose stroke covers it (RING only); entries already >= 0 come from an earlier pass and stay.
// With RING a pixel under a stroke needs no fill any more: its win[k] may stay -1.
template <int NP, bool RING>
__device__ __forceinline__ void walk_list(const DrawList& L, int n, const int4* __restrict__ bx, const float* __restrict__ m, int S, float thr,
                                          int w, long q0, int grow, int shrink, int (&win)[NP], int (&ring)[NP])
{
    const int ya = (int)(q0 / w), xa = (int)(q0 - (long)ya * w);
    const int yb = (int)((q0 + NP - 1) / w);
    for (int e = 0; e < n; ++e) {
        bool open = false;
#pragma unroll
        for (int k = 0; k < NP; ++k) open |= (RING ? ring[k] : win[k]) < 0;
        if (!open) break;
        const int4 b = L.box[e];
        if (b.x - grow > yb || b.z + grow <= ya) continue;
        const int i = L.row[e];
        int y = ya, x = xa;
        PasteRow r = paste_row(bx, m, S, i, y);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if (RING && ring[k] < 0 && in_ring(b, grow, shrink, y, x)) ring[k] = i;
            if (win[k] < 0 && (!RING || ring[k] < 0) && paste_pixel(r, S, x, thr)) win[k] = i;
            if (k < NP - 1 && ++x == w) {
                x = 0; ++y;
                r = paste_row(bx, m, S, i, y);
            }
        }
    }
}

// The same decision for ONE pixel without a list (the few loose bytes around an image's whole chunks): every row of the image.
template <bool RING>
__device__ __forceinline__ void decide_pixel(const int4* __restrict__ bx, const float* __restrict__ det, const float* __restrict__ m, int rows, int S,
                                             float thr, float min_score, int grow, int shrink, int y, int x, int& win, int& ring)
{
    win = ring = -1;
    for (int i = 0; i < rows; ++i) {
        const int4 b = bx[i];
        if (!(b.z > b.x && b.w > b.y && det[(size_t)i * 6 + 5] > min_score)) continue;
        if (RING && in_ring(b, grow, shrink, y, x)) { ring = i; break; }
        if (win < 0) {
            const PasteRow r = paste_row(bx, m, S, i, y);
            if (paste_pixel(r, S, x, thr)) { win = i; if (!RING) break; }
        }
    }
}

// the tile's rectangle from its first and last pixel: whole rows unless it lies inside one
struct TileRect { int y0, y1, x0, x1; };
__device__ __forceinline__ TileRect tile_rect(long qlo, long qhi, int w)
{
    TileRect t;
    t.y0 = (int)(qlo / w); t.y1 = (int)(qhi / w);
    const bool one = t.y0 == t.y1;
    t.x0 = one ? (int)(qlo - (long)t.y0 * w) : 0;
    t.x1 = one ? (int)(qhi - (long)t.y1 * w) : w - 1;
    return t;
}

// ------------------------------------------------------------------------------------------------
// Instance-id map: int16 per pixel, -1 = background.  Algorithmic bytes: 2·h·w written per image.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_instance_map(const ImageGeom* __restrict__ tab, const int4* __restrict__ boxes, const float* __restrict__ det,
                                                      const float* __restrict__ masks, int rows, int S, float thr, float min_score,
                                                      uint8_t* __restrict__ out, uint32_t* __restrict__ visible)
{
    __shared__ DrawList L;
    __shared__ uint32_t s_cnt[DRAW_ROWS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const ImageGeom im = tab[b];
    const int w = im.w;
    const long npix = (long)im.h * w, len = npix * 2;
    uint8_t* const o = out + im.offset;
    const int4* const bx = boxes + (size_t)b * rows;
    const float* const d = det + (size_t)b * rows * 6;
    const float* const m = masks + (size_t)b * rows * S * S;
    uint32_t* const vis = visible ? visible + (size_t)b * rows : nullptr;
    // [0, head) loose | whole 16-byte aligned chunks of 8 pixels | loose   (the base is 2-byte aligned: head is even)
    const long mis = (long)(reinterpret_cast<uintptr_t>(o) & 15);
    const long head = mis ? (16 - mis < len ? 16 - mis : len) : 0;
    const long head_px = head >> 1, chunks = (len - head) >> 4;
    const long tiles = (chunks + 255) >> 8;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long c0 = t << 8, c = c0 + tid;
        const long c1 = c0 + 256 < chunks ? c0 + 256 : chunks;
        const bool live = c < chunks;
        const long q0 = head_px + (live ? c : c0) * 8;
        const TileRect tr = tile_rect(head_px + c0 * 8, head_px + c1 * 8 - 1, w);
        int win[8], none[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) win[k] = none[k] = -1;
        for (int base = 0; base < rows; base += DRAW_ROWS) {
            s_cnt[tid] = 0;
            const int n = cull_rows(L, bx, d, rows, base, min_score, 0, tr.y0, tr.y1, tr.x0, tr.x1);
            if (live) walk_list<8, false>(L, n, bx, m, S, thr, w, q0, 0, 0, win, none);
            if (vis) {
                if (live) {                                             // this pass's winners: rows >= base
                    int cur = -1;
                    uint32_t run = 0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int v = win[k] >= base ? win[k] : -1;
                        if (v != cur) {
                            if (cur >= 0) atomicAdd(&s_cnt[cur - base], run);
                            cur = v; run = 0;
                        }
                        ++run;
                    }
                    if (cur >= 0) atomicAdd(&s_cnt[cur - base], run);
                }
                __syncthreads();
                if (s_cnt[tid]) atomicAdd(&vis[base + tid], s_cnt[tid]);
            }
            __syncthreads();                                            // (the next pass writes the list and the counters)
        }
        if (live) {
            uint32_t q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = ((uint32_t)win[2 * k] & 0xffffu) | ((uint32_t)win[2 * k + 1] << 16);
            *reinterpret_cast<uint4*>(o + head + (c << 4)) = make_uint4(q[0], q[1], q[2], q[3]);
        }
    }
    if (blockIdx.x == 0) {
        const long tail_px = head_px + chunks * 8;
        const long loose = head_px + (npix - tail_px);                  // < 16
        if ((long)tid < loose) {
            const long p = (long)tid < head_px ? (long)tid : tail_px + ((long)tid - head_px);
            const int y = (int)(p / w), x = (int)(p - (long)y * w);
            int win, ring;
            decide_pixel<false>(bx, d, m, rows, S, thr, min_score, 0, 0, y, x, win, ring);
            reinterpret_cast<int16_t*>(o)[p] = (int16_t)win;
            if (vis && win >= 0) atomicAdd(&vis[win], 1u);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Rendered overlay: RGB8.  Algorithmic bytes: 3·h·w read + 3·h·w written per image.
// ------------------------------------------------------------------------------------------------
// The colours and the blend are draw_rule.h's palette_bits, pixel_code and render_byte.

// One tile of 256 lanes × 48 bytes; R = (the first byte of every lane's 48) mod 3, the same for the whole image.
template <int R, bool RING>
__device__ __forceinline__ void render_tile(DrawList& L, const int4* __restrict__ bx, const float* __restrict__ d, const float* __restrict__ m,
                                            int rows, int S, float thr, float min_score, int alpha, int grow, int shrink, int w,
                                            const uint8_t* __restrict__ src, uint8_t* __restrict__ o, long head, long chunks, long t, bool src16)
{
    constexpr int NP = R ? 17 : 16;                                     // the pixels a lane's 48 bytes touch
    const int tid = threadIdx.x;
    const long c0 = t << 8, c = c0 + tid;
    const long c1 = c0 + 256 < chunks ? c0 + 256 : chunks;
    const bool live = c < chunks;
    const long p0 = head + (live ? c : c0) * 48;
    const long q0 = p0 / 3;                                             // p0 = 3 q0 + R
    const TileRect tr = tile_rect((head + c0 * 48) / 3, (head + c1 * 48 - 1) / 3, w);
    // the source first: its latency hides behind the cull and the walk
    uint32_t s[12];
    if (live) {
        if (src16) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + p0 + 16 * k);
                s[4 * k] = v.x; s[4 * k + 1] = v.y; s[4 * k + 2] = v.z; s[4 * k + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k)
                s[k] = (uint32_t)src[p0 + 4 * k] | ((uint32_t)src[p0 + 4 * k + 1] << 8) | ((uint32_t)src[p0 + 4 * k + 2] << 16) | ((uint32_t)src[p0 + 4 * k + 3] << 24);
        }
    }
    int win[NP], ring[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) win[k] = ring[k] = -1;
    for (int base = 0; base < rows; base += DRAW_ROWS) {
        const int n = cull_rows(L, bx, d, rows, base, min_score, grow, tr.y0, tr.y1, tr.x0, tr.x1);
        if (live) walk_list<NP, RING>(L, n, bx, m, S, thr, w, q0, grow, shrink, win, ring);
        __syncthreads();                                                // (the next pass, or the next tile, writes the list)
    }
    if (!live) return;
    uint32_t q[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) q[k] = 0;
#pragma unroll
    for (int j = 0; j < 48; ++j) {
        const int k = (j + R) / 3, ch = (j + R) % 3;
        const uint32_t sb = (s[j >> 2] >> (8 * (j & 3))) & 0xffu;
        q[j >> 2] |= render_byte(sb, pixel_code(win[k], ring[k]), ch, alpha) << (8 * (j & 3));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<uint4*>(o + p0 + 16 * k) = make_uint4(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3]);
}

template <bool RING>
__global__ __launch_bounds__(256) void k_render_detections(const ImageGeom* __restrict__ tab, const int4* __restrict__ boxes, const float* __restrict__ det,
                                                           const float* __restrict__ masks, const uint8_t* const* __restrict__ srcs, int rows, int S,
                                                           float thr, float min_score, int alpha, int grow, int shrink, uint8_t* __restrict__ out)
{
    __shared__ DrawList L;
    const int b = blockIdx.y, tid = threadIdx.x;
    const ImageGeom im = tab[b];
    const int w = im.w;
    const long len = (long)im.h * w * 3;
    uint8_t* const o = out + im.offset;
    const uint8_t* const src = srcs[b];
    const int4* const bx = boxes + (size_t)b * rows;
    const float* const d = det + (size_t)b * rows * 6;
    const float* const m = masks + (size_t)b * rows * S * S;
    // [0, head) loose bytes | whole 48-byte pieces from a 16-byte aligned address | loose bytes
    const long mis = (long)(reinterpret_cast<uintptr_t>(o) & 15);
    const long head = mis ? (16 - mis < len ? 16 - mis : len) : 0;
    const long chunks = (len - head) / 48;
    const long tiles = (chunks + 255) >> 8;
    const bool src16 = (reinterpret_cast<uintptr_t>(src + head) & 15) == 0;
    const int R = (int)(head % 3);
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        if (R == 0) render_tile<0, RING>(L, bx, d, m, rows, S, thr, min_score, alpha, grow, shrink, w, src, o, head, chunks, t, src16);
        else if (R == 1) render_tile<1, RING>(L, bx, d, m, rows, S, thr, min_score, alpha, grow, shrink, w, src, o, head, chunks, t, src16);
        else render_tile<2, RING>(L, bx, d, m, rows, S, thr, min_score, alpha, grow, shrink, w, src, o, head, chunks, t, src16);
    }
    if (blockIdx.x == 0) {
        const long tail0 = head + chunks * 48;
        const long loose = head + (len - tail0);                        // < 16 + 48
        if ((long)tid < loose) {
            const long p = (long)tid < head ? (long)tid : tail0 + ((long)tid - head);
            const long px = p / 3;
            const int ch = (int)(p - px * 3);
            const int y = (int)(px / w), x = (int)(px - (long)y * w);
            int win, ring;
            decide_pixel<RING>(bx, d, m, rows, S, thr, min_score, grow, shrink, y, x, win, ring);
            o[p] = (uint8_t)render_byte(src[p], pixel_code(win, ring), ch, alpha);
        }
    }
}

static int tile_grid(long max_chunks)
{
    const long tiles = (max_chunks + 255) / 256;
    return (int)(tiles < 1 ? 1 : (tiles < 1024 ? tiles : 1024));
}

void instance_map_forward(hipStream_t s, const float* det, const float* masks, const ImageGeom* tab, int batch, int rows, int S, int H, int W,
                          long max_pixels, float thr, float min_score, float* det_src, int4* boxes, int16_t* map, uint32_t* visible)
{
    if (batch <= 0) return;
    unletterbox_boxes_forward(s, det, tab, batch, rows, H, W, det_src, boxes);
    if (visible && rows > 0) HIP_CHECK(hipMemsetAsync(visible, 0, (size_t)batch * rows * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_instance_map, dim3(tile_grid(max_pixels / 8), batch), dim3(256), 0, s, tab, boxes, det, masks, rows, S, thr, min_score,
                       reinterpret_cast<uint8_t*>(map), visible);
    HIP_CHECK(hipGetLastError());
}

void render_detections_forward(hipStream_t s, const float* det, const float* masks, const ImageGeom* tab, const uint8_t* const* srcs, int batch,
                               int rows, int S, int H, int W, long max_pixels, float thr, float min_score, int alpha, int stroke, float* det_src,
                               int4* boxes, uint8_t* out)
{
    if (batch <= 0) return;
    unletterbox_boxes_forward(s, det, tab, batch, rows, H, W, det_src, boxes);
    const int grow = stroke / 2, shrink = stroke - stroke / 2;
    const dim3 grid(tile_grid(max_pixels / 16), batch);
    if (stroke > 0)
        hipLaunchKernelGGL(k_render_detections<true>, grid, dim3(256), 0, s, tab, boxes, det, masks, srcs, rows, S, thr, min_score, alpha, grow, shrink, out);
    else
        hipLaunchKernelGGL(k_render_detections<false>, grid, dim3(256), 0, s, tab, boxes, det, masks, srcs, rows, S, thr, min_score, alpha, 0, 0, out);
    HIP_CHECK(hipGetLastError());
}

}  // namespace mrcnn

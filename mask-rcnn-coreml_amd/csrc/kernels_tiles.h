// kernels_tiles.h — the launches of mrcnn_merge_tiles and mrcnn_unite_tiles (kernels_tiles.hip).  Every table is a device array.
#pragma once
#include "kernels.h"

namespace mrcnn {

struct TileGeom { int image, y0, x0, img_h, img_w, th, tw; };  // one tile: its image, its origin there, that image's size, the window's own size

// The candidates of both entries are the rows of every tile: candidate k = t*rows + i.
struct TilesMerge {
    int n_tiles, rows, S, n_images, max_out, W;                // W = 64-bit words of a suppression row: ceil(largest candidates per image / 64)
    float thr; int metric; double match_thr;                   // (match_thr: the merge's match threshold / the union's link threshold)
    const float* det; const float* masks;                      // (n_tiles, rows, 6) in the letterboxed frame of each tile, (n_tiles, rows, S, S)
    const TileGeom* tiles;                                     // n_tiles
    const ImageGeom* tab_full;                                 // n_tiles: h / w of the tile's IMAGE (what the RLE kernels read)
    const int* toff; const int* tlist;                         // tiles of image b, ascending: tlist[toff[b] .. toff[b+1])
    const int2* imgsz;                                         // n_images: (h, w)
    // scratch
    int4* boxes; float* rows_src;                              // per candidate: full-frame pixel box ((0,0,0,0) = not eligible), source-frame row
    RleSeg* segs; uint32_t* nruns; long long* ro; uint32_t* areas; int32_t* bboxes; uint32_t* counts;   // the candidates' RLEs in the full frame
    int* order; int* pos; int* nelig;                          // per image: candidates by (score desc, k asc); a candidate's place there, -1 = not eligible
    unsigned long long* supp;                                  // (n_tiles*rows, W): bit r of row c = the candidate at place r < pos[c] suppresses c if kept
                                                               // (the union: … is linked with c)
    uint32_t* out_nruns;                                       // n_images*max_out
    // scratch of the union only
    int* members; int2* mspan;                                 // the candidates grouped by component, in place order (n_tiles*rows, laid out like
                                                               // `order`); per slot its members [x, y) there
    int4* hull; RleSeg* out_segs;                              // per slot: the hull of its members' boxes; the segments of its union walk
    // outputs (device)
    float* det_src; int32_t* source; int32_t* n_kept; long long* out_ro; uint32_t* out_areas; int32_t* out_bboxes; uint32_t* out_counts;
    int32_t* n_parts; int32_t* group;                          // the union only: n_images*max_out, n_tiles*rows
};

// boxes must hold the tile-frame pixel boxes (unletterbox_boxes_forward with the tiles' own geometry).  Shifts them into the full frame,
// writes rows_src, then counts the runs of every candidate plane: m.ro[n_tiles*rows] = the size m.counts needs.
void tiles_rle_count_forward(hipStream_t s, const TilesMerge& m);
// m.counts allocated: the candidates' runs and the per-image order.  Shared by the merge and the union.
void tiles_order_forward(hipStream_t s, const TilesMerge& m);
// the merge: the suppression bits, the greedy scan and the size of the output: m.out_ro[n_images*max_out] = the size out_counts needs.
// det_src, source, n_kept, out_ro, out_areas, out_bboxes are final.
void tiles_select_forward(hipStream_t s, const TilesMerge& m);
// the runs of the kept candidates into m.out_counts
void tiles_gather_forward(hipStream_t s, const TilesMerge& m);
// the union: the link bits, the components, the union planes counted: m.out_ro[n_images*max_out] = the size out_counts needs.
// det_src, source, n_kept, n_parts, group, out_ro, out_areas, out_bboxes are final.
void tiles_unite_forward(hipStream_t s, const TilesMerge& m);
// the runs of the union planes into m.out_counts
void tiles_unite_write_forward(hipStream_t s, const TilesMerge& m);

}  // namespace mrcnn

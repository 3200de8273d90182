// kernels_jpeg_entropy.h — the launches of the entropy stage (kernels_jpeg_entropy.hip), for api_jpeg.hip alone: the other translation
// units never see the decoding step.
#pragma once
#include "common.h"
#include "jpeg_entropy.h"

namespace mrcnn {

// ================================================================================================
// JPEG entropy decoding on the device (kernels_jpeg_entropy.hip; the decoding step is jpeg_entropy.h's, shared with the host model)
// ================================================================================================
// The device buffers of one call.  files .. bytes: the plan of jpeg_entropy_host.h's plan_entropy and the files' bytes, uploaded; the rest
// is written by the launches: state / wg_exit / wg_entry start as all ones (ENT_INVALID), count / prefix / wg_flags / verdict as zeros.
// verdict: {status bits, last launch that changed something} per file, then the most rounds a workgroup ran.
struct JpegEntBuffers {
    const jpeg::EntFile* files;
    const jpeg::EntSeg* segs;
    const int32_t* unit_seg;
    const jpeg::EntWg* wgs;
    const uint8_t* bytes;
    unsigned long long* state;       // nunits
    unsigned long long* wg_exit;     // 2 * nwg
    unsigned long long* wg_entry;    // nwg
    uint32_t* count;                 // nunits
    uint32_t* prefix;                // nunits + 1
    int32_t* wg_flags;               // 2 * nwg: converged inside, rounds so far
    int32_t* verdict;                // 2 * batch + 1
    int batch, nsegs, nunits, nwg, unit_bytes, launches, inner_rounds;
};
// One fill, `launches` synchronisation launches (jpeg_entropy.h's ent_launches: from the sizes of the files, never from their content),
// then the scan, the writing pass and the DC predictors.  coef: the array jpeg_decode_forward reads, cleared here.
void jpeg_entropy_forward(hipStream_t s, const JpegEntBuffers& b, int16_t* coef, long long total_blocks);

}  // namespace mrcnn

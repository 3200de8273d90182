// jpeg_entropy_host.h — the host side of the self-synchronising entropy stage (jpeg_entropy.h): the marker scan that cuts the scans of
// a batch into segments, units and workgroups (byte-level only: no bit of the stream is decoded here), and the sequential MODEL of the
// device phases, which runs the same step function launch for launch, workgroup for workgroup, round for round.  Plain C++17, no HIP.
#pragma once
#include <vector>

#include "jpeg_entropy.h"
#include "jpeg_host.h"

namespace mrcnn {
namespace jpeg {

struct EntropyPlan {
    int unit_bytes = ENT_UNIT_BYTES;
    std::vector<EntFile> files;
    std::vector<EntSeg> segs;
    std::vector<int32_t> unit_seg;      // unit -> segment
    std::vector<EntWg> wgs;
    long long blob_bytes = 0;           // the files' bytes, each from a multiple of 16
    int max_file_wgs = 0;
};

// The marker scan.  block0[b]: the file's first block in the batch's coefficient array.  A file whose scan is not "segments of entropy
// data, RST0..7 in order between them, EOI behind the last" gets nseg = 0: the host decoder decides about it.
void plan_entropy(const mrcnn_jpeg* files, const Header* hdr, const long long* block0, int batch, int unit_bytes, EntropyPlan& plan);

// clean = the verdict: the coefficients of the file are what decode_coefficients writes (and it accepts the file)
inline bool ent_clean(const EntFile& f, int status, int last_change, int launches)
{
    return f.nseg > 0 && status == 0 && (f.nunits == 1 || (launches >= 2 && last_change < launches));
}

// The model: coef (the batch's array, total_blocks * 64) is cleared and written like the device does; clean[b] as above; *rounds = the
// most rounds a workgroup ran over all launches.
void entropy_model(const EntropyPlan& plan, const mrcnn_jpeg* files, int max_rounds, int16_t* coef, long long total_blocks, std::vector<char>& clean,
                   int* rounds);

}  // namespace jpeg
}  // namespace mrcnn

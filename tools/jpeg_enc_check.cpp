// jpeg_enc_check.cpp — the host JPEG encoder (csrc/jpeg_enc_host.cpp) under the sanitizers, as a program of its own:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I mask-rcnn-coreml_amd/csrc \
//       tools/jpeg_enc_check.cpp mask-rcnn-coreml_amd/csrc/jpeg_enc_host.cpp mask-rcnn-coreml_amd/csrc/jpeg_host.cpp -o jpeg_enc_check
//   ./jpeg_enc_check
//
// Host code only: no GPU, no HIP, no Python.  It sweeps every size 1x1 .. 40x40, the four samplings and qualities 1 / 50 / 100 over
// seeded images (noise, so that the largest size categories occur, and a smooth ramp, so that long zero runs do).  Each image is
// encoded three times — the size query, a buffer one byte short, a buffer of exactly the size reported (so a write past it is a
// report) — and the file is fed to the host decoder with an output buffer of exactly h*w*3 bytes.  Exit status: 0 = clean; 1 = a
// status, a size or a decoded shape was not what the protocol promises; a sanitizer report ends the program with the sanitizer's own
// non-zero status.
#include <stdio.h>

#include <string>
#include <vector>

#include "jpeg_enc_host.h"
#include "jpeg_host.h"

using namespace mrcnn;

int main()
{
    int bad = 0;
    long runs = 0;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (int h = 1; h <= 40; ++h)
        for (int w = 1; w <= 40; ++w) {
            // an exact-size copy of the pixels: a read past h*w*3 is a read past the allocation
            std::vector<uint8_t> rgb((size_t)h * w * 3);
            const bool noise = (h + w) % 2 == 0;
            for (size_t i = 0; i < rgb.size(); ++i) {
                seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                rgb[i] = noise ? (uint8_t)(seed >> 56) : (uint8_t)((i / 3 % (size_t)w) * 5 + (i / 3 / (size_t)w) * 3 + i % 3 * 40);
            }
            for (int sampling = 0; sampling < 4; ++sampling)
                for (int quality : {1, 50, 100}) {
                    ++runs;
                    std::string err;
                    int64_t need = -1, n = -1;
                    if (jpeg::encode_host(rgb.data(), h, w, quality, sampling, nullptr, 0, &need, &err) != MRCNN_OK || need < 300) {       // (a grey header alone is over 300 bytes)
                        printf("%dx%d s%d q%d: size query failed (%s)\n", h, w, sampling, quality, err.c_str());
                        ++bad;
                        continue;
                    }
                    std::vector<uint8_t> small((size_t)need - 1, 0xAB);
                    if (jpeg::encode_host(rgb.data(), h, w, quality, sampling, small.data(), need - 1, &n, &err) != MRCNN_ERR_SHAPE || n != need ||
                        small[0] != 0xAB || small.back() != 0xAB) {
                        printf("%dx%d s%d q%d: a buffer one byte short was not refused untouched\n", h, w, sampling, quality);
                        ++bad;
                    }
                    std::vector<uint8_t> file((size_t)need);
                    if (jpeg::encode_host(rgb.data(), h, w, quality, sampling, file.data(), need, &n, &err) != MRCNN_OK || n != need) {
                        printf("%dx%d s%d q%d: encode failed (%s)\n", h, w, sampling, quality, err.c_str());
                        ++bad;
                        continue;
                    }
                    jpeg::Header hd;
                    std::vector<uint8_t> back((size_t)h * w * 3);
                    if (jpeg::parse(file.data(), need, &hd, &err) != MRCNN_OK || hd.height != h || hd.width != w || hd.components != (sampling == 3 ? 1 : 3) ||
                        jpeg::decode_host(file.data(), need, back.data(), (int64_t)back.size(), &err) != MRCNN_OK) {
                        printf("%dx%d s%d q%d: the decoder does not take the file back (%s)\n", h, w, sampling, quality, err.c_str());
                        ++bad;
                    }
                }
        }
    printf("%ld encodes, %d findings\n", runs, bad);
    return bad ? 1 : 0;
}

// jpeg_entropy_check.cpp — the self-synchronising entropy stage's host model (csrc/jpeg_entropy_host.cpp, the step function of
// csrc/jpeg_entropy.h that the kernels run too) under the sanitizers, as a program of its own:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I mask-rcnn-coreml_amd/csrc \
//       tools/jpeg_entropy_check.cpp mask-rcnn-coreml_amd/csrc/jpeg_entropy_host.cpp mask-rcnn-coreml_amd/csrc/jpeg_host.cpp -o jpeg_entropy_check
//   ./jpeg_entropy_check <dir with the fixture files>
//
// Host code only: no GPU, no HIP, no Python.  For every file of the directory, EVERY truncation of it (every third where the file is
// larger than 16 KB, every one of its last 64) and 200 seeded single-byte
// corruptions it runs the marker scan and, where that finds segments, the model at unit sizes 4, 16 and 128 on an exact-size copy of the data (a read past the length is a report) and
// into a coefficient array of exactly the header's size.  Exit status 1 unless model-plus-fallback equals decode_coefficients: a file
// the model calls clean must be accepted by decode_coefficients with the same coefficients (every other file IS decode_coefficients'
// answer); an intact file that decodes must also be clean — no fallback.  A sanitizer report ends the program with its own status.
#include <dirent.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "jpeg_entropy_host.h"

using namespace mrcnn;

static long g_models = 0, g_clean = 0, g_scans = 0;

// 0 = agrees; 1 = a finding.  *host_status: what decode_coefficients says (parse failures included)
static int check(const std::vector<uint8_t>& bytes, size_t length, bool must_be_clean, const char* what, int* host_status)
{
    std::vector<uint8_t> data(bytes.begin(), bytes.begin() + (long)length);
    jpeg::Header h;
    std::string err;
    int st = jpeg::parse(data.data(), (int64_t)data.size(), &h, &err);
    *host_status = st;
    if (st != MRCNN_OK) return 0;                                  // (no entropy stage runs on a refused header)
    if (h.total_blocks > (int64_t)1 << 20) return 0;               // (a corrupted size field: not this program's business)
    const mrcnn_jpeg file = {data.data(), (int64_t)data.size()};
    const long long block0 = 0;
    if (!must_be_clean) {           // a file the marker scan hands to the host decoder IS the host decoder's answer: nothing to compare
        jpeg::EntropyPlan probe;
        jpeg::plan_entropy(&file, &h, &block0, 1, 128, probe);
        ++g_scans;
        if (probe.files[0].nseg == 0) return 0;
    }
    std::vector<int16_t> want((size_t)h.total_blocks * 64), got((size_t)h.total_blocks * 64);
    st = jpeg::decode_coefficients(data.data(), (int64_t)data.size(), h, want.data(), &err);
    *host_status = st;
    int bad = 0;
    for (int unit : {4, 16, 128}) {
        jpeg::EntropyPlan plan;
        jpeg::plan_entropy(&file, &h, &block0, 1, unit, plan);
        std::vector<char> clean;
        int rounds = 0;
        jpeg::entropy_model(plan, &file, 0, got.data(), h.total_blocks, clean, &rounds);
        ++g_models;
        if (clean[0]) {
            ++g_clean;
            if (st != MRCNN_OK) { printf("%s, unit %d: the model calls clean what decode_coefficients refuses (%d: %s)\n", what, unit, st, err.c_str()); ++bad; }
            else if (memcmp(want.data(), got.data(), want.size() * sizeof(int16_t)) != 0) { printf("%s, unit %d: clean, but the coefficients differ\n", what, unit); ++bad; }
        } else if (must_be_clean && st == MRCNN_OK) {
            printf("%s, unit %d: an intact file fell back (%d rounds)\n", what, unit, rounds);
            ++bad;
        }
    }
    return bad;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <dir with JPEG files>\n", argv[0]); return 64; }
    std::vector<std::string> names;
    if (DIR* d = opendir(argv[1])) {
        while (dirent* e = readdir(d))
            if (e->d_name[0] != '.') names.push_back(e->d_name);
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    if (names.empty()) { fprintf(stderr, "%s: no files\n", argv[1]); return 66; }
    int bad = 0;
    long runs = 0;
    for (const std::string& name : names) {
        const std::string path = std::string(argv[1]) + "/" + name;
        std::vector<uint8_t> bytes;
        if (FILE* f = fopen(path.c_str(), "rb")) {
            uint8_t buf[4096];
            size_t n;
            while ((n = fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
            fclose(f);
        }
        if (bytes.empty()) { fprintf(stderr, "%s: cannot read\n", path.c_str()); return 66; }
        int whole = 0, st = 0;
        bad += check(bytes, bytes.size(), true, name.c_str(), &whole);
        ++runs;
        char what[300];
        const size_t stride = bytes.size() > 16384 ? 3 : 1;       // (a larger file: every third truncation, and every one of the last 64)
        for (size_t k = 0; k < bytes.size(); k += k + 64 >= bytes.size() ? 1 : stride, ++runs) {
            snprintf(what, sizeof what, "%s truncated to %zu bytes", name.c_str(), k);
            bad += check(bytes, k, false, what, &st);
        }
        uint64_t seed = 0x9E3779B97F4A7C15ull ^ bytes.size();
        for (int i = 0; i < 200; ++i, ++runs) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            const size_t at = (size_t)((seed >> 33) % bytes.size());
            const uint8_t keep = bytes[at];
            bytes[at] = (uint8_t)(keep ^ (uint8_t)(1 + ((seed >> 20) % 255)));
            snprintf(what, sizeof what, "%s corruption %d (byte %zu)", name.c_str(), i, at);
            bad += check(bytes, bytes.size(), false, what, &st);
            bytes[at] = keep;
        }
        printf("%s: %zu bytes, intact -> %d\n", name.c_str(), bytes.size(), whole);
    }
    printf("%ld inputs, %ld marker scans, %ld model runs (%ld clean), %d findings\n", runs, g_scans, g_models, g_clean, bad);
    return bad ? 1 : 0;
}

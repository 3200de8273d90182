// jpeg_host_check.cpp — the JPEG parser and entropy decoder (csrc/jpeg_host.cpp) under the sanitizers, as a program of its own:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I mask-rcnn-coreml_amd/csrc \
//       tools/jpeg_host_check.cpp mask-rcnn-coreml_amd/csrc/jpeg_host.cpp -o jpeg_host_check
//   ./jpeg_host_check <dir with the fixture files>
//
// Host code only: no GPU, no HIP, no Python.  For every file of the directory it runs decode_host over the file, over EVERY
// truncation of it and over 200 seeded single-byte corruptions, each time with an output buffer of exactly the size the header
// names (so a write past it is a report).  Exit status: 0 = clean; 1 = a truncation was accepted as a whole file, or an intact file
// returned a status other than OK / UNSUPPORTED; a sanitizer report ends the program with the sanitizer's own non-zero status.
#include <dirent.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "jpeg_host.h"

using namespace mrcnn;

static int decode(const std::vector<uint8_t>& bytes, size_t length, std::string* err)
{
    // an exact-size copy: a read past `length` is a read past the allocation
    std::vector<uint8_t> data(bytes.begin(), bytes.begin() + (long)length);
    jpeg::Header h;
    int st = jpeg::parse(data.data(), (int64_t)data.size(), &h, err);
    if (st != MRCNN_OK) return st;
    const int64_t need = (int64_t)h.height * h.width * 3;
    if (need > (int64_t)1 << 26) return MRCNN_ERR_SHAPE;          // (a corrupted size field: not this program's business)
    std::vector<uint8_t> rgb((size_t)need);
    st = jpeg::decode_host(data.data(), (int64_t)data.size(), rgb.data(), need, err);
    if (st == MRCNN_OK && need > 0) {
        std::vector<uint8_t> small((size_t)need - 1);
        std::string e2;
        if (jpeg::decode_host(data.data(), (int64_t)data.size(), small.data(), need - 1, &e2) != MRCNN_ERR_SHAPE) return -1;
    }
    return st;
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
        std::string err;
        const int whole = decode(bytes, bytes.size(), &err);
        ++runs;
        if (whole != MRCNN_OK && whole != MRCNN_ERR_UNSUPPORTED) { printf("%s: intact file -> status %d (%s)\n", name.c_str(), whole, err.c_str()); ++bad; }
        for (size_t k = 0; k < bytes.size(); ++k, ++runs) {
            const int st = decode(bytes, k, &err);
            if (st != MRCNN_ERR_IO && st != MRCNN_ERR_UNSUPPORTED) { printf("%s: truncation to %zu bytes -> status %d\n", name.c_str(), k, st); ++bad; }
        }
        uint64_t seed = 0x9E3779B97F4A7C15ull ^ bytes.size();
        for (int i = 0; i < 200; ++i, ++runs) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            const size_t at = (size_t)((seed >> 33) % bytes.size());
            const uint8_t keep = bytes[at];
            bytes[at] = (uint8_t)(keep ^ (uint8_t)(1 + ((seed >> 20) % 255)));
            const int st = decode(bytes, bytes.size(), &err);
            bytes[at] = keep;
            if (st < MRCNN_OK || st > MRCNN_ERR_CONFIG) { printf("%s: corruption %d -> status %d\n", name.c_str(), i, st); ++bad; }
        }
        printf("%s: %zu bytes, intact -> %d\n", name.c_str(), bytes.size(), whole);
    }
    printf("%ld decodes, %d findings\n", runs, bad);
    return bad ? 1 : 0;
}

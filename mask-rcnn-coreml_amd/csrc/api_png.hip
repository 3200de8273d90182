// api_png.hip — the C ABI of include/maskrcnn_hip.h, PNG files out: the host entry (png_host.cpp behind it) and the device entry.  A
// batch is encoded in one pass over one device allocation: the descriptor table and the host-built chunks go up in a single copy,
// kernels_png.hip runs its launches, the file offsets come back (the capacity check), then only the files' bytes.
//
// IDAT's CRC-32 is filled in HERE, on the host, after the copy: the files are host memory by contract, a label file is a few KB, and
// the table CRC of png_host.cpp is at hand — zlib is not linked.  The device leaves the four bytes zero.
#include <string.h>

#include <mutex>

#include "api_util.h"
#include "png_format.h"
#include "png_host.h"

using namespace mrcnn;

static_assert(MRCNN_PNG_GREY8 == png::FORMAT_GREY8 && MRCNN_PNG_INSTANCE == png::FORMAT_INSTANCE && MRCNN_PNG_BLOCK_BYTES == png::PNG_BLOCK_BYTES,
              "png_format.h restates the header's constants");

extern "C" int mrcnn_png_encode_host(const void* pixels, int height, int width, int format, int rows, uint8_t* out, int64_t capacity,
                                     int64_t* length)
{
    return guarded([&] {
        std::string err;
        const int st = png::encode_host(pixels, height, width, format, rows, out, capacity, length, &err);
        if (st != MRCNN_OK) fail(st, "%s", err.c_str());
    });
}

namespace {

// mrcnn_png_encode_batch has no handle to keep its scratch in: one grow-only allocation per process, handed to one call at a time.
// Never freed — at process exit the HIP runtime may be gone before a static destructor would run.
DevBuf& shared_scratch() { static DevBuf* b = new DevBuf; return *b; }
std::mutex g_scratch_mutex;

}  // namespace

extern "C" int mrcnn_png_encode_batch(const mrcnn_png_source* images, int batch, int memspace, int format, int rows, uint8_t* out,
                                      int64_t capacity, int64_t* file_offsets)
{
    return guarded([&] {
        // every argument error before the device is touched
        MRCNN_REQUIRE(images && file_offsets && capacity >= 0 && (out || capacity == 0), MRCNN_ERR_INVALID,
                      "png_encode_batch: null pointer or negative capacity");
        std::string err;
        if (const int st = png::check_format(format, rows, "png_encode_batch", &err)) fail(st, "%s", err.c_str());
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "png_encode_batch: unknown memspace %d", memspace);
        MRCNN_REQUIRE(batch >= 1 && batch <= MRCNN_PNG_MAX_BATCH, MRCNN_ERR_SHAPE, "png_encode_batch: batch %d outside 1..%d", batch, MRCNN_PNG_MAX_BATCH);
        for (int b = 0; b < batch; ++b) {
            char who[64];
            snprintf(who, sizeof who, "png_encode_batch: image %d of the batch", b);
            if (const int st = png::check_image(images[b].pixels, images[b].height, images[b].width, who, &err)) fail(st, "%s", err.c_str());
        }
        require_gpu();

        // the layout of the call's one allocation
        const size_t sample = format == MRCNN_PNG_INSTANCE ? 2 : 1;
        std::vector<PngDesc> desc((size_t)batch);
        std::vector<uint8_t> headers;
        long long total_blocks = 0, files_capacity = 0;
        size_t pixel_bytes = 0;
        for (int b = 0; b < batch; ++b) {
            const int h = images[b].height, w = images[b].width;
            const std::vector<uint8_t> hd = png::header(h, w, format, rows);
            PngDesc& d = desc[(size_t)b];
            memset(&d, 0, sizeof d);
            d.n = (long long)h * (w + 1);
            d.block0 = total_blocks; d.blocks = (d.n + png::PNG_BLOCK_BYTES - 1) / png::PNG_BLOCK_BYTES;
            d.h = h; d.w = w;
            d.header0 = (int)headers.size(); d.header_len = (int)hd.size();
            headers.insert(headers.end(), hd.begin(), hd.end());
            total_blocks += d.blocks;
            files_capacity += png::max_file_bytes(h, w, hd.size());
            pixel_bytes += memspace == MRCNN_HOST ? up(sample * h * w, 16) : 0;
        }
        files_capacity = (long long)up((size_t)files_capacity, 4);
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += up(bytes, 256); return o; };
        const size_t o_tab = take((size_t)batch * sizeof(PngDesc)), o_hdr = take(headers.size());
        const size_t upload = at;
        const size_t o_pix = take(pixel_bytes), o_bits = take((size_t)total_blocks * 4), o_scan = take((size_t)(total_blocks + 1) * 8);
        const size_t o_adler = take((size_t)batch * 16), o_off = take((size_t)(batch + 1) * 8), o_files = take((size_t)files_capacity);

        std::lock_guard<std::mutex> lock(g_scratch_mutex);
        DevBuf& sc = shared_scratch();
        if (sc.bytes < at) sc.alloc(at);
        uint8_t* const base = sc.as<uint8_t>();
        if (memspace == MRCNN_HOST) {
            size_t o = o_pix;
            for (int b = 0; b < batch; ++b) {
                desc[(size_t)b].pixels = base + o;
                o += up(sample * images[b].height * images[b].width, 16);
            }
        } else {
            for (int b = 0; b < batch; ++b) desc[(size_t)b].pixels = images[b].pixels;
        }
        std::vector<uint8_t> staged(upload, 0);
        memcpy(staged.data() + o_tab, desc.data(), (size_t)batch * sizeof(PngDesc));
        memcpy(staged.data() + o_hdr, headers.data(), headers.size());

        Stream st;
        Drain drain{st.s};
        HIP_CHECK(hipMemcpyAsync(base, staged.data(), upload, hipMemcpyHostToDevice, st.s));
        if (memspace == MRCNN_HOST)
            for (int b = 0; b < batch; ++b)
                HIP_CHECK(hipMemcpyAsync(const_cast<void*>(desc[(size_t)b].pixels), images[b].pixels, sample * images[b].height * images[b].width,
                                         hipMemcpyHostToDevice, st.s));
        PngBuffers buf;
        buf.tab = reinterpret_cast<const PngDesc*>(base + o_tab);
        buf.headers = base + o_hdr;
        buf.block_bits = reinterpret_cast<uint32_t*>(base + o_bits);
        buf.block_scan = reinterpret_cast<unsigned long long*>(base + o_scan);
        buf.adler = reinterpret_cast<unsigned long long*>(base + o_adler);
        buf.file_offsets = reinterpret_cast<long long*>(base + o_off);
        buf.files = reinterpret_cast<uint32_t*>(base + o_files);
        buf.files_capacity = files_capacity;
        png_encode_forward(st.s, buf, batch, total_blocks, format, rows);
        static_assert(sizeof(long long) == sizeof(int64_t), "file offsets are copied as they are");
        HIP_CHECK(hipMemcpyAsync(file_offsets, buf.file_offsets, (size_t)(batch + 1) * 8, hipMemcpyDeviceToHost, st.s));
        HIP_CHECK(hipStreamSynchronize(st.s));
        const int64_t need = file_offsets[batch];
        bool sane = need >= 0 && need <= files_capacity && file_offsets[0] == 0;
        for (int b = 0; b < batch && sane; ++b)
            sane = file_offsets[b + 1] - file_offsets[b] >= desc[(size_t)b].header_len + png::IDAT_LEAD + png::IDAT_TAIL + png::IEND_BYTES;
        MRCNN_REQUIRE(sane, MRCNN_ERR_HIP, "png_encode_batch: the device reported %lld bytes of files, beyond the %lld possible, or a file without its frame",
                      (long long)need, files_capacity);
        if (capacity == 0 && !out) return;              // the size query
        MRCNN_REQUIRE(need <= capacity, MRCNN_ERR_SHAPE, "png_encode_batch: the %d files need a capacity of %lld bytes, the buffer holds %lld", batch,
                      (long long)need, (long long)capacity);
        HIP_CHECK(hipMemcpy(out, buf.files, (size_t)need, hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; ++b) {               // IDAT's CRC-32: over its type and data, stored big-endian before IEND
            uint8_t* const type = out + file_offsets[b] + desc[(size_t)b].header_len + 4;
            uint8_t* const crc_at = out + file_offsets[b + 1] - png::IEND_BYTES - 4;
            const uint32_t crc = png::crc32(0, type, (size_t)(crc_at - type));
            for (int k = 0; k < 4; ++k) crc_at[k] = (uint8_t)(crc >> (24 - 8 * k));
        }
    });
}

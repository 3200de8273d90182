// api_jpeg_enc.hip — the C ABI of include/maskrcnn_hip.h, JPEG files out: the host entry (jpeg_enc_host.cpp behind it) and the device
// entry.  A batch is encoded in one pass over one device allocation: the descriptor table, the code tables and the headers go up in a
// single copy, kernels_jpeg_enc.hip runs its launches, the file offsets come back (the capacity check), then only the files' bytes.
#include <string.h>

#include <mutex>

#include "api_util.h"
#include "jpeg_enc_host.h"

using namespace mrcnn;

extern "C" int mrcnn_jpeg_encode_host(const uint8_t* rgb, int height, int width, int quality, int sampling, uint8_t* out, int64_t capacity,
                                      int64_t* length)
{
    return guarded([&] {
        std::string err;
        const int st = jpeg::encode_host(rgb, height, width, quality, sampling, out, capacity, length, &err);
        if (st != MRCNN_OK) fail(st, "%s", err.c_str());
    });
}

namespace {

// mrcnn_jpeg_encode_batch has no handle to keep its scratch in: one grow-only allocation per process, handed to one call at a time.
// Never freed — at process exit the HIP runtime may be gone before a static destructor would run.
DevBuf& shared_scratch() { static DevBuf* b = new DevBuf; return *b; }
std::mutex g_scratch_mutex;

static_assert(sizeof(JpegEncHuffman) == sizeof(jpeg::EncHuffman) + 64, "JpegEncHuffman = EncHuffman + the zigzag table");

}  // namespace

extern "C" int mrcnn_jpeg_encode_batch(const mrcnn_image* images, int batch, int memspace, int quality, int sampling, uint8_t* out,
                                       int64_t capacity, int64_t* file_offsets)
{
    return guarded([&] {
        // every argument error before the device is touched
        MRCNN_REQUIRE(images && file_offsets && capacity >= 0 && (out || capacity == 0), MRCNN_ERR_INVALID,
                      "jpeg_encode_batch: null pointer or negative capacity");
        MRCNN_REQUIRE(sampling >= MRCNN_JPEG_444 && sampling <= MRCNN_JPEG_GREY, MRCNN_ERR_INVALID, "jpeg_encode_batch: unknown sampling %d", sampling);
        MRCNN_REQUIRE(memspace == MRCNN_HOST || memspace == MRCNN_DEVICE, MRCNN_ERR_INVALID, "jpeg_encode_batch: unknown memspace %d", memspace);
        MRCNN_REQUIRE(batch >= 1 && batch <= MRCNN_JPEG_MAX_BATCH, MRCNN_ERR_SHAPE, "jpeg_encode_batch: batch %d outside 1..%d", batch, MRCNN_JPEG_MAX_BATCH);
        MRCNN_REQUIRE(quality >= 1 && quality <= 100, MRCNN_ERR_SHAPE, "jpeg_encode_batch: quality %d outside 1..100", quality);
        for (int b = 0; b < batch; ++b) {
            MRCNN_REQUIRE(images[b].rgb, MRCNN_ERR_INVALID, "jpeg_encode_batch: image %d of the batch: null rgb", b);
            MRCNN_REQUIRE(images[b].height >= 1 && images[b].height <= 32767 && images[b].width >= 1 && images[b].width <= 32767, MRCNN_ERR_SHAPE,
                          "jpeg_encode_batch: image %d of the batch is %dx%d: height and width must lie in 1..32767", b, images[b].height, images[b].width);
        }
        require_gpu();

        // the layout of the call's one allocation
        std::vector<JpegEncDesc> desc((size_t)batch);
        std::vector<uint8_t> headers;
        uint16_t quant[2][64];
        jpeg::enc_quant_tables(quality, quant);
        long long total_blocks = 0, max_chunks = 0, files_capacity = 0;
        size_t rgb_bytes = 0;
        for (int b = 0; b < batch; ++b) {
            const int h = images[b].height, w = images[b].width;
            const jpeg::EncGeometry g = jpeg::enc_geometry(h, w, sampling);
            const std::vector<uint8_t> hd = jpeg::enc_header(h, w, quality, sampling);
            JpegEncDesc& d = desc[(size_t)b];
            memset(&d, 0, sizeof d);
            d.block0 = total_blocks; d.blocks = g.blocks;
            d.h = h; d.w = w; d.sampling = sampling; d.ncomp = g.ncomp;
            d.hs = g.hs; d.vs = g.vs; d.mcus_x = g.mcus_x; d.blocks_per_mcu = g.blocks_per_mcu;
            d.header0 = (int)headers.size(); d.header_len = (int)hd.size();
            memcpy(d.quant, quant, sizeof quant);
            headers.insert(headers.end(), hd.begin(), hd.end());
            total_blocks += g.blocks;
            const long long chunks = (g.blocks * JPEG_ENC_BLOCK_BYTES + JPEG_ENC_CHUNK - 1) / JPEG_ENC_CHUNK;
            max_chunks += chunks;
            files_capacity += (long long)hd.size() + 2 + 2 * chunks * JPEG_ENC_CHUNK;      // (every byte of a scan may be an FF)
            rgb_bytes += memspace == MRCNN_HOST ? up((size_t)3 * h * w, 16) : 0;
        }
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += up(bytes, 256); return o; };
        const size_t o_tab = take((size_t)batch * sizeof(JpegEncDesc)), o_huff = take(sizeof(JpegEncHuffman)), o_hdr = take(headers.size());
        const size_t upload = at;
        const size_t o_rgb = take(rgb_bytes), o_coef = take((size_t)total_blocks * 128), o_bits = take((size_t)total_blocks * 4);
        const size_t o_bscan = take((size_t)(total_blocks + 1) * 8), o_c0 = take((size_t)(batch + 1) * 8), o_bytes = take((size_t)batch * 8);
        const size_t o_stream = take((size_t)max_chunks * JPEG_ENC_CHUNK), o_ff = take((size_t)max_chunks * 4), o_cscan = take((size_t)(max_chunks + 1) * 8);
        const size_t o_off = take((size_t)(batch + 1) * 8), o_files = take((size_t)files_capacity);

        std::lock_guard<std::mutex> lock(g_scratch_mutex);
        DevBuf& sc = shared_scratch();
        if (sc.bytes < at) sc.alloc(at);
        uint8_t* const base = sc.as<uint8_t>();
        if (memspace == MRCNN_HOST) {
            size_t o = o_rgb;
            for (int b = 0; b < batch; ++b) {
                desc[(size_t)b].rgb = base + o;
                o += up((size_t)3 * images[b].height * images[b].width, 16);
            }
        } else {
            for (int b = 0; b < batch; ++b) desc[(size_t)b].rgb = images[b].rgb;
        }
        std::vector<uint8_t> staged(upload, 0);
        memcpy(staged.data() + o_tab, desc.data(), (size_t)batch * sizeof(JpegEncDesc));
        JpegEncHuffman huff;
        memcpy(&huff, &jpeg::enc_huffman(), sizeof(jpeg::EncHuffman));
        for (int k = 0; k < 64; ++k) huff.zigzag_of[jpeg::kZigzag[k]] = (uint8_t)k;
        memcpy(staged.data() + o_huff, &huff, sizeof huff);
        memcpy(staged.data() + o_hdr, headers.data(), headers.size());

        Stream st;
        Drain drain{st.s};
        HIP_CHECK(hipMemcpyAsync(base, staged.data(), upload, hipMemcpyHostToDevice, st.s));
        if (memspace == MRCNN_HOST)
            for (int b = 0; b < batch; ++b)
                HIP_CHECK(hipMemcpyAsync(const_cast<uint8_t*>(desc[(size_t)b].rgb), images[b].rgb, (size_t)3 * images[b].height * images[b].width,
                                         hipMemcpyHostToDevice, st.s));
        JpegEncBuffers buf;
        buf.tab = reinterpret_cast<const JpegEncDesc*>(base + o_tab);
        buf.huff = reinterpret_cast<const JpegEncHuffman*>(base + o_huff);
        buf.headers = base + o_hdr;
        buf.coef = reinterpret_cast<int16_t*>(base + o_coef);
        buf.block_bits = reinterpret_cast<uint32_t*>(base + o_bits);
        buf.block_scan = reinterpret_cast<unsigned long long*>(base + o_bscan);
        buf.image_chunk0 = reinterpret_cast<long long*>(base + o_c0);
        buf.image_bytes = reinterpret_cast<long long*>(base + o_bytes);
        buf.stream = reinterpret_cast<uint32_t*>(base + o_stream);
        buf.chunk_ff = reinterpret_cast<uint32_t*>(base + o_ff);
        buf.chunk_scan = reinterpret_cast<unsigned long long*>(base + o_cscan);
        buf.file_offsets = reinterpret_cast<long long*>(base + o_off);
        buf.files = base + o_files;
        buf.max_chunks = max_chunks;
        buf.files_capacity = files_capacity;
        jpeg_encode_forward(st.s, buf, batch, total_blocks);
        static_assert(sizeof(long long) == sizeof(int64_t), "file offsets are copied as they are");
        HIP_CHECK(hipMemcpyAsync(file_offsets, buf.file_offsets, (size_t)(batch + 1) * 8, hipMemcpyDeviceToHost, st.s));
        HIP_CHECK(hipStreamSynchronize(st.s));
        const int64_t need = file_offsets[batch];
        MRCNN_REQUIRE(need >= 0 && need <= files_capacity, MRCNN_ERR_HIP, "jpeg_encode_batch: the device reported %lld bytes of files, beyond the %lld possible",
                      (long long)need, files_capacity);
        if (capacity == 0 && !out) return;              // the size query
        MRCNN_REQUIRE(need <= capacity, MRCNN_ERR_SHAPE, "jpeg_encode_batch: the %d files need a capacity of %lld bytes, the buffer holds %lld", batch,
                      (long long)need, (long long)capacity);
        HIP_CHECK(hipMemcpy(out, buf.files, (size_t)need, hipMemcpyDeviceToHost));
    });
}

// engine_weights.hip — the .mrcw reader, BatchNorm folding and the weight packers: everything between an artefact's bytes and a
// PackedConv on the device.
#include "engine_internal.h"
#include "conv_pack.h"

#include <math.h>
#include <string.h>

#include <fstream>

namespace mrcnn {

// ------------------------------------------------------------------------------------------------
// .mrcw
// ------------------------------------------------------------------------------------------------
float half_to_float(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu, f;
    if (exp == 0) {
        if (man == 0) f = sign;
        else {
            exp = 113;
            while ((man & 0x400u) == 0) { man <<= 1; --exp; }
            man &= 0x3FFu;
            f = sign | (exp << 23) | (man << 13);
        }
    } else if (exp == 31) f = sign | 0x7F800000u | (man << 13);
    else f = sign | ((exp + 112) << 23) | (man << 13);
    float r;
    memcpy(&r, &f, 4);
    return r;
}

void MrcwFile::load(const std::string& p)
{
    path = p;
    std::ifstream in(p, std::ios::binary | std::ios::ate);
    MRCNN_REQUIRE(in.good(), MRCNN_ERR_IO, "cannot open model artefact '%s'", p.c_str());
    const std::streamsize sz = in.tellg();
    in.seekg(0);
    buf.resize((size_t)sz);
    in.read(reinterpret_cast<char*>(buf.data()), sz);
    MRCNN_REQUIRE(in.good() && sz >= 16 && memcmp(buf.data(), "MRCW", 4) == 0, MRCNN_ERR_IO, "'%s' is not a .mrcw file", p.c_str());
    size_t pos = 4;
    auto need = [&](size_t n) { MRCNN_REQUIRE(pos + n <= buf.size(), MRCNN_ERR_IO, "'%s': truncated header", p.c_str()); };
    auto rd = [&](void* dst, size_t n) { need(n); memcpy(dst, buf.data() + pos, n); pos += n; };
    uint32_t ver, n_meta, n_t;
    rd(&ver, 4); rd(&n_meta, 4); rd(&n_t, 4);
    MRCNN_REQUIRE(ver == 1, MRCNN_ERR_IO, "'%s': unsupported .mrcw version %u", p.c_str(), ver);
    for (uint32_t i = 0; i < n_meta; ++i) {
        uint16_t kl; rd(&kl, 2);
        need(kl);
        std::string k((const char*)buf.data() + pos, kl); pos += kl;
        uint8_t t; rd(&t, 1);
        if (t == 0) { int64_t v; rd(&v, 8); ints[k] = v; }
        else if (t == 1) { double v; rd(&v, 8); doubles[k] = v; }
        else { uint32_t sl; rd(&sl, 4); need(sl); strings[k] = std::string((const char*)buf.data() + pos, sl); pos += sl; }
    }
    struct Ent { std::string name; MrcwTensor t; uint64_t off; };
    std::vector<Ent> ents;
    for (uint32_t i = 0; i < n_t; ++i) {
        uint16_t nl; rd(&nl, 2);
        need(nl);
        Ent e;
        e.name = std::string((const char*)buf.data() + pos, nl); pos += nl;
        uint8_t dt, nd; rd(&dt, 1); rd(&nd, 1);
        e.t.dtype = dt;
        e.t.dims.resize(nd);
        for (int d = 0; d < nd; ++d) rd(&e.t.dims[d], 4);
        uint64_t nb; rd(&e.off, 8); rd(&nb, 8);
        e.t.nbytes = (size_t)nb;
        ents.push_back(std::move(e));
    }
    const size_t base = (pos + 63) / 64 * 64;
    for (auto& e : ents) {
        MRCNN_REQUIRE(base + e.off + e.t.nbytes <= buf.size(), MRCNN_ERR_IO, "'%s': tensor %s out of bounds", p.c_str(), e.name.c_str());
        MRCNN_REQUIRE(e.t.dtype == 0 || e.t.dtype == 2, MRCNN_ERR_IO, "'%s': tensor %s has unsupported dtype", p.c_str(), e.name.c_str());
        e.t.data = buf.data() + base + e.off;
        tensors[e.name] = e.t;
    }
}
int64_t MrcwFile::get_int(const std::string& k) const
{
    auto it = ints.find(k);
    MRCNN_REQUIRE(it != ints.end(), MRCNN_ERR_IO, "'%s': missing integer metadata key '%s'", path.c_str(), k.c_str());
    return it->second;
}
int64_t MrcwFile::get_int(const std::string& k, int64_t dflt) const
{
    auto it = ints.find(k);
    return it == ints.end() ? dflt : it->second;
}
double MrcwFile::get_double(const std::string& k, double dflt) const
{
    auto it = doubles.find(k);
    if (it != doubles.end()) return it->second;
    auto ii = ints.find(k);
    return ii == ints.end() ? dflt : (double)ii->second;
}
std::string MrcwFile::get_string(const std::string& k) const
{
    auto it = strings.find(k);
    MRCNN_REQUIRE(it != strings.end(), MRCNN_ERR_IO, "'%s': missing string metadata key '%s'", path.c_str(), k.c_str());
    return it->second;
}
const MrcwTensor& MrcwFile::tensor(const std::string& name) const
{
    auto it = tensors.find(name);
    MRCNN_REQUIRE(it != tensors.end(), MRCNN_ERR_IO, "'%s': missing tensor '%s'", path.c_str(), name.c_str());
    return it->second;
}
std::vector<float> MrcwFile::floats(const std::string& name) const
{
    const MrcwTensor& t = tensor(name);
    std::vector<float> v(t.count());
    if (t.dtype == 0) memcpy(v.data(), t.data, v.size() * 4);
    else {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(t.data);
        for (size_t i = 0; i < v.size(); ++i) v[i] = half_to_float(h[i]);
    }
    return v;
}

// ------------------------------------------------------------------------------------------------
// weight packing
// ------------------------------------------------------------------------------------------------
void upload(DevBuf& d, const std::vector<float>& h)
{
    d.alloc(h.size() * 4);
    HIP_CHECK(hipMemcpy(d.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
}

static uint16_t float_to_half(float f)   // round to nearest even
{
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7FFFFFFFu;
    if (x >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | (x > 0x7F800000u ? 0x200u : 0));
    if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);            // overflow → inf
    if (x < 0x38800000u) {                                              // subnormal half / zero
        if (x < 0x33000000u) return (uint16_t)sign;
        const int e = (int)(x >> 23);
        uint32_t m = (x & 0x7FFFFFu) | 0x800000u;
        const int shift = 126 - e;                                      // 14..24
        const uint32_t half_m = m >> shift, rem = m & ((1u << shift) - 1), mid = 1u << (shift - 1);
        uint32_t r = half_m;
        if (rem > mid || (rem == mid && (half_m & 1))) ++r;
        return (uint16_t)(sign | r);
    }
    uint32_t r = ((x - 0x38000000u) >> 13);
    const uint32_t rem = x & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) ++r;
    return (uint16_t)(sign | r);
}

// filter weights in the compute dtype (the artefact stores fp16, so the fp16 path is lossless)
static void upload_w(DevBuf& d, const std::vector<float>& h, int dtype, bool must_be_exact = false, const char* what = "")
{
    if (dtype != MRCNN_F16 && dtype != MRCNN_F32X3) { upload(d, h); return; }
    std::vector<uint16_t> hh(h.size());
    for (size_t i = 0; i < h.size(); ++i) {
        hh[i] = float_to_half(h[i]);
        if (must_be_exact) {
            const _Float16 back = __builtin_bit_cast(_Float16, hh[i]);
            MRCNN_REQUIRE((float)back == h[i], MRCNN_ERR_UNSUPPORTED,
                          "%s: filter value %.9g is not fp16-representable; MRCNN_F32S needs the fp16 filters the converter writes", what, h[i]);
        }
    }
    d.alloc(hh.size() * 2);
    HIP_CHECK(hipMemcpy(d.p, hh.data(), hh.size() * 2, hipMemcpyHostToDevice));
}

// scale/shift of conv(+bias)(+BN):  y = acc*scale + shift
static void fold_bn(const MrcwFile& f, const std::string& conv, const std::string& bn, int Cout, int Npad,
                    std::vector<float>& scale, std::vector<float>& shift)
{
    const std::vector<float> bias = f.floats(conv + "/bias");
    MRCNN_REQUIRE((int)bias.size() == Cout, MRCNN_ERR_IO, "%s/bias has %zu entries, expected %d", conv.c_str(), bias.size(), Cout);
    scale.assign(Npad, 0.f);
    shift.assign(Npad, 0.f);
    if (bn.empty()) {
        for (int o = 0; o < Cout; ++o) { scale[o] = 1.f; shift[o] = bias[o]; }
        return;
    }
    const std::vector<float> g = f.floats(bn + "/gamma"), be = f.floats(bn + "/beta"), mu = f.floats(bn + "/mean"),
                             var = f.floats(bn + "/variance");
    const float eps = (float)f.get_double("bn_eps", 1e-3);
    for (int o = 0; o < Cout; ++o) {
        const float sc = g[o] / sqrtf(var[o] + eps);
        scale[o] = sc;
        shift[o] = (bias[o] - mu[o]) * sc + be[o];
    }
}

// What every packer starts and ends with.  new_pack: the element types of the compute mode, the filter shape and Npad = Cout rounded
// up to its N tile.  finish_pack: the filters in the mode's filter type (a split mode insists that they are fp16 values), scale / shift on
// the device and their host copies.
static PackedConv new_pack(int mode, int Cin, int Cout, int KH, int KW)
{
    PackedConv pc;
    pc.dtype = mode_act(mode); pc.wdtype = mode_wgt(mode);
    pc.Cin = Cin; pc.Cout = Cout; pc.KH = KH; pc.KW = KW;
    const int bn_tile = conv_n_tile(Cout);
    pc.Npad = (Cout + bn_tile - 1) / bn_tile * bn_tile;
    return pc;
}
static void finish_pack(PackedConv& pc, const std::vector<float>& w, const std::vector<float>& sc, const std::vector<float>& sh)
{
    upload_w(pc.wgt, w, pc.wdtype, pc.wdtype != pc.dtype, "MRCNN_F32S / MRCNN_F32X3");
    upload(pc.scale, sc);
    upload(pc.shift, sh);
    pc.h_scale = sc; pc.h_shift = sh;
}

// kernel [O][I][KH][KW] (Core ML layout) → [Npad][KH][KW][I]
PackedConv pack_conv_oihw(const MrcwFile& f, const std::string& conv, const std::string& bn, int dtype)
{
    const MrcwTensor& t = f.tensor(conv + "/kernel");
    MRCNN_REQUIRE(t.dims.size() == 4, MRCNN_ERR_IO, "%s/kernel is not 4-D", conv.c_str());
    const int O = t.dims[0], I = t.dims[1], KH = t.dims[2], KW = t.dims[3];
    const std::vector<float> k = f.floats(conv + "/kernel");
    PackedConv pc = new_pack(dtype, I, O, KH, KW);
    const std::vector<float> w = pack_filter_rows(O, I, KH, KW, pc.Npad, [&](int o, int y, int x, int i) { return k[(((size_t)o * I + i) * KH + y) * KW + x]; });
    std::vector<float> sc, sh;
    fold_bn(f, conv, bn, O, pc.Npad, sc, sh);
    finish_pack(pc, w, sc, sh);
    if (pc.wdtype != pc.dtype && conv_halo_packable(KH, KW, I, pc.Npad)) {
        conv_halo_pack(nullptr, pc.wgt.p, pc.Npad, I, pc.wgt_halo);           // split modes: also in the halo kernel's tiling
        HIP_CHECK(hipStreamSynchronize(nullptr));
    } else if (pc.wdtype != pc.dtype && conv_halo_tail_packable(KH, KW, I, pc.Npad) && O == pc.Npad) {
        conv_halo_pack(nullptr, pc.wgt.p, pc.Npad, I, pc.wgt_halo, 1);        // ... the 256 -> 1024 1x1 layers for the fused bottleneck tail
        HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    if (pc.wdtype != pc.dtype && pc.dtype == MRCNN_F32 && O == pc.Npad && chain_stream_wanted(KH, KW, I, O) && conv.find("_branch2") != std::string::npos) {
        // split modes, the bottlenecks' 256 <-> 1024 pointwise layers (C4): also as the chained pair's stream image, built once here
        std::vector<uint16_t> hw(w.size());
        for (size_t i = 0; i < w.size(); ++i) hw[i] = float_to_half(w[i]);
        const std::vector<uint16_t> img = pack_chain_stream(hw.data(), 256, I == 1024);
        pc.wgt_stream.alloc(img.size() * 2);
        HIP_CHECK(hipMemcpy(pc.wgt_stream.p, img.data(), img.size() * 2, hipMemcpyHostToDevice));
    }
    if (pc.dtype == MRCNN_F16 && pc.wdtype == MRCNN_F16 && conv3x3h_packable(KH, KW, I, O, pc.Npad)) {
        conv3x3h_pack(nullptr, pc.wgt.p, O, I, pc.wgt_c3h);
        HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    if (pc.dtype == MRCNN_F16 && pc.wdtype == MRCNN_F16 && O == pc.Npad && bneck_frag_wanted(KH, KW, I, O)) {
        bneck_pack_frag(nullptr, pc.wgt.p, O, KH * KW * I, pc.wgt_frag);      // fp16 mode: C4's identity bottlenecks stream these straight into registers
        HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    return pc;
}

// conv1: 7×7 stride 2 on 3 channels.  The input is staged as zero-padded NHWC4, so one kernel row
// (7 taps × 4 channels = 28 floats, padded to 32) is a contiguous 128-B run: taps = 7 (rows),
// "Cin" = 32.  Packed [64][7][32] with k = kw*4 + ci.
PackedConv pack_conv1(const MrcwFile& f, int dtype)
{
    const MrcwTensor& t = f.tensor("conv1/kernel");
    MRCNN_REQUIRE(t.dims.size() == 4 && t.dims[1] == 3 && t.dims[2] == 7 && t.dims[3] == 7, MRCNN_ERR_IO, "conv1/kernel must be [O,3,7,7]");
    const int O = t.dims[0];
    const std::vector<float> k = f.floats("conv1/kernel");
    const int px = mode_act(dtype) == MRCNN_F16 ? 8 : 4;   // channels per staged pixel (NHWC8 / NHWC4): 16 B either way
    const int row = 8 * px;                         // one kernel row = 7 taps padded to 8 pixels = 128 B
    PackedConv pc = new_pack(dtype, row, O, 7, 1);
    std::vector<float> w((size_t)pc.Npad * 7 * row, 0.f);
    for (int o = 0; o < O; ++o)
        for (int ci = 0; ci < 3; ++ci)
            for (int y = 0; y < 7; ++y)
                for (int x = 0; x < 7; ++x)
                    w[((size_t)o * 7 + y) * row + x * px + ci] = k[(((size_t)o * 3 + ci) * 7 + y) * 7 + x];
    std::vector<float> sc, sh;
    fold_bn(f, "conv1", "bn_conv1", O, pc.Npad, sc, sh);
    finish_pack(pc, w, sc, sh);
    return pc;
}

// Several [O_i][I] inner-product / 1×1 kernels stacked along N (no BN).
PackedConv pack_stacked_1x1(const MrcwFile& f, const std::vector<std::string>& names, int dtype)
{
    int O = 0, I = -1;
    for (auto& n : names) {
        const MrcwTensor& t = f.tensor(n + "/kernel");
        MRCNN_REQUIRE(t.dims.size() == 2 || (t.dims.size() == 4 && t.dims[2] == 1 && t.dims[3] == 1), MRCNN_ERR_IO,
                      "%s/kernel is not an inner product / 1x1 kernel", n.c_str());
        MRCNN_REQUIRE(I < 0 || I == (int)t.dims[1], MRCNN_ERR_IO, "%s: input size mismatch", n.c_str());
        I = t.dims[1];
        O += t.dims[0];
    }
    PackedConv pc = new_pack(dtype, I, O, 1, 1);
    std::vector<float> w((size_t)pc.Npad * I, 0.f), sc(pc.Npad, 0.f), sh(pc.Npad, 0.f);
    int o0 = 0;
    for (auto& n : names) {
        const std::vector<float> k = f.floats(n + "/kernel"), b = f.floats(n + "/bias");
        memcpy(w.data() + (size_t)o0 * I, k.data(), k.size() * 4);
        for (size_t o = 0; o < b.size(); ++o) { sc[o0 + o] = 1.f; sh[o0 + o] = b[o]; }
        o0 += (int)b.size();
    }
    finish_pack(pc, w, sc, sh);
    return pc;
}

// ConvTranspose 2×2 stride 2, kernel [I][O][2][2] → GEMM rows n = (dy*2+dx)*O + co.
PackedConv pack_deconv2(const MrcwFile& f, const std::string& name, int dtype)
{
    const MrcwTensor& t = f.tensor(name + "/kernel");
    MRCNN_REQUIRE(t.dims.size() == 4 && t.dims[2] == 2 && t.dims[3] == 2, MRCNN_ERR_IO, "%s/kernel must be [I,O,2,2]", name.c_str());
    const int I = t.dims[0], O = t.dims[1];
    const std::vector<float> k = f.floats(name + "/kernel"), b = f.floats(name + "/bias");
    PackedConv pc = new_pack(dtype, I, O, 1, 1);
    pc.Npad = 4 * O;                              // (four GEMM rows per output channel: not the rounded-up Cout)
    MRCNN_REQUIRE(pc.Npad % conv_n_tile(pc.Npad) == 0, MRCNN_ERR_SHAPE, "%s: 4*O must be a multiple of the N tile", name.c_str());
    const std::vector<float> w = pack_deconv2_rows(I, O, pc.Npad, [&](int dy, int dx, int o, int i) { return k[(((size_t)i * O + o) * 2 + dy) * 2 + dx]; });
    std::vector<float> sc(pc.Npad, 1.f), sh(pc.Npad);
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx)
            for (int o = 0; o < O; ++o) sh[(size_t)deconv2_row(dy, dx, o, O)] = b[o];
    finish_pack(pc, w, sc, sh);
    return pc;
}

// A convolution's own copy of its scale / shift (= the folded BatchNorm + bias until exponents are applied)
void init_scaled_op(ScaledOp& op, const PackedConv* pc, int g_in, int g_out)
{
    op.pc = pc; op.g_in = g_in; op.g_out = g_out;
    upload(op.scale, pc->h_scale);
    upload(op.shift, pc->h_shift);
}

}  // namespace mrcnn

// jpeg_entropy_host.cpp — see jpeg_entropy_host.h.  Plain C++17, no HIP.
#include "jpeg_entropy_host.h"

#include <string.h>

namespace mrcnn {
namespace jpeg {

namespace {

// the FF that ends the entropy data starting at `from`: the first one not followed by 00; -1 = none before the end of the data
int64_t segment_end(const uint8_t* data, int64_t length, int64_t from)
{
    int64_t p = from;
    while (p < length) {
        const void* f = memchr(data + p, 0xFF, (size_t)(length - p));
        if (!f) return -1;
        p = (const uint8_t*)f - data;
        if (p + 1 < length && data[p + 1] == 0x00) { p += 2; continue; }
        return p;
    }
    return -1;
}

}  // namespace

void plan_entropy(const mrcnn_jpeg* files, const Header* hdr, const long long* block0, int batch, int unit_bytes, EntropyPlan& plan)
{
    plan.unit_bytes = unit_bytes > 0 ? unit_bytes : ENT_UNIT_BYTES;
    const int U = plan.unit_bytes;
    plan.files.assign((size_t)batch, EntFile());
    plan.segs.clear(); plan.unit_seg.clear(); plan.wgs.clear();
    plan.blob_bytes = 0; plan.max_file_wgs = 0;
    for (int b = 0; b < batch; ++b) {
        const Header& h = hdr[b];
        const uint8_t* const data = files[b].data;
        const int64_t length = files[b].length;
        EntFile& f = plan.files[(size_t)b];
        memset(&f, 0, sizeof f);
        f.byte0 = plan.blob_bytes;
        f.length = length;
        plan.blob_bytes += (length + 15) / 16 * 16;
        f.ncomp = h.components;
        f.hs = h.h_samp; f.vs = h.v_samp;
        f.nluma = h.components == 1 ? 1 : h.h_samp * h.v_samp;
        f.bpm = h.components == 1 ? 1 : f.nluma + 2;
        f.mcus_x = h.mcus_x; f.mcus_y = h.mcus_y;
        for (int c = 0; c < h.components; ++c) {
            f.comp_block0[c] = block0[b] + h.comp[c].block0;
            f.comp_blocks_w[c] = h.comp[c].blocks_w;
            build_huff_table(h.dc[h.comp[c].td], f.tab[c]);
            build_huff_table(h.ac[h.comp[c].ta], f.tab[3 + c]);
        }
        f.seg0 = (int)plan.segs.size();
        f.unit0 = (int)plan.unit_seg.size();
        f.wg0 = (int)plan.wgs.size();
        // the marker scan
        const int64_t mcus = (int64_t)h.mcus_x * h.mcus_y, R = h.restart_interval ? h.restart_interval : mcus;
        const int64_t nseg = (mcus + R - 1) / R;
        bool ok = f.bpm <= ENT_MAX_BPM && length < ((int64_t)1 << 28) && nseg < ((int64_t)1 << 24) &&
                  (int64_t)plan.unit_seg.size() + length / U + nseg < ((int64_t)1 << 30);
        int64_t pos = h.scan_offset;
        for (int64_t k = 0; ok && k < nseg; ++k) {
            const int64_t end = segment_end(data, length, pos);
            if (end <= pos || end + 1 >= length) { ok = false; break; }          // no marker, or no entropy data in front of it
            const int want = k + 1 == nseg ? 0xD9 : 0xD0 + (int)(k & 7);
            if (data[end + 1] != want) { ok = false; break; }                    // (a fill byte FF included)
            EntSeg s;
            memset(&s, 0, sizeof s);
            s.b0 = pos; s.b1 = end;
            s.first_block = k * R * f.bpm;
            s.nblocks = (int)((k + 1 == nseg ? mcus - k * R : R) * f.bpm);
            s.file = b;
            s.unit0 = (int)plan.unit_seg.size();
            s.nunits = (int)((end - pos + U - 1) / U);
            plan.unit_seg.insert(plan.unit_seg.end(), (size_t)s.nunits, (int32_t)plan.segs.size());
            plan.segs.push_back(s);
            pos = end + 2;
        }
        if (!ok) {
            plan.segs.resize((size_t)f.seg0);
            plan.unit_seg.resize((size_t)f.unit0);
            continue;
        }
        f.nseg = (int)plan.segs.size() - f.seg0;
        f.nunits = (int)plan.unit_seg.size() - f.unit0;
        for (int u = 0; u < f.nunits; u += ENT_WG_UNITS) {
            EntWg w;
            w.file = b; w.unit0 = f.unit0 + u; w.count = f.nunits - u < ENT_WG_UNITS ? f.nunits - u : ENT_WG_UNITS; w.reserved = 0;
            plan.wgs.push_back(w);
        }
        f.nwg = (int)plan.wgs.size() - f.wg0;
        if (f.nwg > plan.max_file_wgs) plan.max_file_wgs = f.nwg;
    }
}

void entropy_model(const EntropyPlan& plan, const mrcnn_jpeg* files, int max_rounds, int16_t* coef, long long total_blocks, std::vector<char>& clean,
                   int* rounds)
{
    const int batch = (int)plan.files.size(), U = plan.unit_bytes;
    const size_t nunits = plan.unit_seg.size(), nwg = plan.wgs.size();
    const int launches = ent_launches(U, plan.max_file_wgs, max_rounds), inner = ent_inner_rounds(max_rounds);
    std::vector<ent_state> state(nunits, ENT_INVALID), wg_exit[2], wg_entry(nwg, ENT_INVALID);
    wg_exit[0].assign(nwg, ENT_INVALID); wg_exit[1].assign(nwg, ENT_INVALID);
    std::vector<int> count(nunits, 0), wg_done(nwg, 0), wg_rounds(nwg, 0), status((size_t)batch, 0), last_change((size_t)batch, 0);
    // phase 1: synchronisation
    for (int launch = 0; launch < launches; ++launch) {
        const int cur = launch & 1, prev = cur ^ 1;
        for (size_t w = 0; w < nwg; ++w) {
            const EntWg& g = plan.wgs[w];
            const EntFile& f = plan.files[(size_t)g.file];
            const ent_state entry = launch > 0 && (int)w > f.wg0 ? wg_exit[prev][w - 1] : ENT_INVALID;
            if (launch > 0 && wg_done[w] && entry == wg_entry[w]) { wg_exit[cur][w] = wg_exit[prev][w]; continue; }
            wg_entry[w] = entry;
            std::vector<ent_state> st[2];
            st[0].assign(state.begin() + g.unit0, state.begin() + g.unit0 + g.count);
            st[1] = st[0];
            std::vector<int> cnt(count.begin() + g.unit0, count.begin() + g.unit0 + g.count);
            std::vector<ent_state> last_in((size_t)g.count, ENT_INVALID);
            int at = 0, any = 1, n = 0;
            while (n < inner && any) {
                any = 0;
                for (int t = 0; t < g.count; ++t) {
                    const int u = g.unit0 + t;
                    const EntSeg& s = plan.segs[(size_t)plan.unit_seg[(size_t)u]];
                    const EntUnit q = ent_unit(s, u, U);
                    const EntCtx c = ent_ctx(f, s, files[g.file].data, f.tab, kZigzag);
                    ent_state in = q.first ? ent_pack(c.b0 * 8, 0, 0) : (t == 0 ? entry : st[at][(size_t)t - 1]);
                    if (in == ENT_INVALID) in = ent_guess(c.data, c.b0, q.ub);
                    if (n > 0 && in == last_in[(size_t)t]) { st[at ^ 1][(size_t)t] = st[at][(size_t)t]; continue; }
                    last_in[(size_t)t] = in;
                    const EntResult r = decode_unit(c, q.ub, q.ue, in, nullptr);
                    if (r.state != st[at][(size_t)t] || r.blocks != cnt[(size_t)t]) any = 1;
                    st[at ^ 1][(size_t)t] = r.state;
                    cnt[(size_t)t] = r.blocks;
                }
                at ^= 1;
                ++n;
            }
            wg_done[w] = !any;
            wg_rounds[w] += n;
            for (int t = 0; t < g.count; ++t) { state[(size_t)(g.unit0 + t)] = st[at][(size_t)t]; count[(size_t)(g.unit0 + t)] = cnt[(size_t)t]; }
            wg_exit[cur][w] = st[at][(size_t)g.count - 1];
            if (any || wg_exit[cur][w] != wg_exit[prev][w] || launch == 0) last_change[(size_t)g.file] = launch + 1;
        }
    }
    // phase 2: block offsets
    std::vector<long long> prefix(nunits + 1, 0);
    for (size_t u = 0; u < nunits; ++u) prefix[u + 1] = prefix[u] + count[u];
    // phase 3: the writing pass
    memset(coef, 0, (size_t)total_blocks * 64 * sizeof(int16_t));
    for (size_t u = 0; u < nunits; ++u) {
        const EntSeg& s = plan.segs[(size_t)plan.unit_seg[u]];
        const EntFile& f = plan.files[(size_t)s.file];
        const EntCtx c = ent_ctx(f, s, files[s.file].data, f.tab, kZigzag);
        const long long p0 = prefix[(size_t)s.unit0];
        status[(size_t)s.file] |= ent_write_unit(c, f, s, (int)u, U, state.data(), prefix[u] - p0, prefix[u + 1] - p0, coef);
    }
    // phase 4: the DC predictors, per component inside each segment, modulo 2^16
    for (const EntSeg& s : plan.segs) {
        const EntFile& f = plan.files[(size_t)s.file];
        const EntSink k = ent_sink(f, coef);
        uint16_t pred[3] = {0, 0, 0};
        for (long long q = s.first_block; q < s.first_block + s.nblocks; ++q) {
            const int b = (int)(q % f.bpm), comp = b < f.nluma ? 0 : b - f.nluma + 1;
            int16_t* dc = coef + ent_block_index(k, q, f.bpm, f.nluma) * 64;
            pred[comp] = (uint16_t)(pred[comp] + (uint16_t)*dc);
            *dc = (int16_t)pred[comp];
        }
    }
    clean.assign((size_t)batch, 0);
    int most = 0;
    for (size_t w = 0; w < nwg; ++w) most = wg_rounds[w] > most ? wg_rounds[w] : most;
    for (int b = 0; b < batch; ++b) {
        const EntFile& f = plan.files[(size_t)b];
        bool synced = true;
        for (int w = f.wg0; w < f.wg0 + f.nwg; ++w) synced = synced && wg_done[(size_t)w];
        clean[(size_t)b] = ent_clean(f, status[(size_t)b] | (synced || f.nunits == 1 ? 0 : ENT_BAD_SYNC), last_change[(size_t)b], launches) ? 1 : 0;
    }
    if (rounds) *rounds = most;
}

}  // namespace jpeg
}  // namespace mrcnn

// Checkpoint packing, host only: the staged tensors (ctx->host, ctx->pitch_table) become the host image of the weight arena, the
// context slots that will point into it, the images' geometry and the analytic bounds the launches take.  No HIP call: api.hip
// uploads the image and resolves the slots.
#include <algorithm>
#include <cmath>

#include "tvc_common.h"

namespace tvc {

size_t ArenaBuilder::put(const float** slot, const float* v, size_t n) {
    const size_t off = (buf.size() + 63) & ~size_t(63);  // 256-byte aligned
    buf.resize(off + n, 0.f);
    std::copy(v, v + n, buf.begin() + off);
    fix.push_back({slot, off});
    return off;
}

namespace {

int pad_m(int M) {
    if (M <= 32) return 32;
    if (M <= 64) return 64;
    if (M <= 96) return 96;
    if (M % 96 == 0 && M % 128 != 0) return M;
    return (M + 127) / 128 * 128;
}

// ---- two-part fp16 split of the packed weights (split_fp16.h): w = (h1 + 2^-11 h2) * 2^e, e per 32-row m-tile -------------------
uint16_t f16_bits(float f) {
    const _Float16 h = (_Float16)f;          // round to nearest even, subnormals kept
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}
float f16_value(uint16_t u) {
    _Float16 h;
    std::memcpy(&h, &u, 2);
    return (float)h;
}
// the two parts of w / scale (scale = a power of two: the division is exact)
void split2(float w, float scale, uint16_t* h1, uint16_t* h2) {
    const float x = w / scale;
    *h1 = f16_bits(x);
    *h2 = f16_bits((x - f16_value(*h1)) * 2048.f);
}
// power of two that brings `amax` into [1, 2) (1 for an all-zero tile)
float pow2_scale(float amax) {
    if (!(amax > 0.f) || !std::isfinite(amax)) return 1.f;
    int e;
    std::frexp(amax, &e);                    // amax = m * 2^e, m in [0.5, 1)
    return std::ldexp(1.f, e - 1);
}
float amax(const float* v, size_t n) {
    float a = 0.f;
    for (size_t i = 0; i < n; ++i) a = std::max(a, std::fabs(v[i]));
    return a;
}
// max_m sum_k |w[m][k]| (summed in double, k ascending) and max_m |b[m]| of a weight [M][K] and its bias [M]: |w x + b| <= w |x|max + b
struct RowL1 {
    double w = 0.0, b = 0.0;
};
RowL1 row_l1(const float* w, const float* b, int M, int K) {
    RowL1 r;
    for (int m = 0; m < M; ++m) {
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum += std::fabs((double)w[(size_t)m * K + k]);
        r.w = std::max(r.w, sum);
        r.b = std::max(r.b, std::fabs((double)b[m]));
    }
    return r;
}

// A weight w [M][CI][taps] (taps = 3, or 1 for a 1x1) in the 24-channel K-unit layout of filter_up24s.hip, two fp16 parts (split2) by
// the per-m-tile scales: K runs in units of (tap, 8-channel group), K16 step s takes unit u = 2 s + (lane >> 5) = (tap u / 3, channel
// ci = 8 (u % 3) + j), row m = 32 mt + (lane & 31).  (step s, m-tile mt) goes to piece piece0 + s * step_stride + 2 mt, its second part
// to the piece behind it.  Units u >= 3 taps, rows m >= M and channels ci >= CI are zero.
void put_k24(std::vector<float>& img, int piece0, int step_stride, const float* w, int M, int CI, int taps, const float* scale) {
    uint16_t* o = reinterpret_cast<uint16_t*>(img.data());
    for (int s = 0; 2 * s < 3 * taps; ++s)
        for (int mt = 0; 32 * mt < M; ++mt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int u = 2 * s + (lane >> 5), tap = u / 3, ci = 8 * (u % 3) + j, m = 32 * mt + (lane & 31);
                    const float v = (u < 3 * taps && m < M && ci < CI) ? w[((size_t)m * CI + ci) * taps + tap] : 0.f;
                    const size_t base = ((size_t)(piece0 + s * step_stride + 2 * mt) * 64 + lane) * 8 + j;
                    split2(v, scale[mt], &o[base], &o[base + 512]);
                }
}

struct Packer {
    tvc_ctx* ctx;
    ArenaBuilder& ab;
    std::string missing;                                           // the first missing or misshapen key
    std::map<const PackedW*, std::vector<float>> host_wscale;      // the scales chosen for every packed image (joint packing, fused-block blobs)

    void note(const std::string& what) {
        if (missing.empty()) missing = what;
    }
    const HostTensor* find(const std::string& key) {
        auto it = ctx->host.find(key);
        if (it != ctx->host.end()) return &it->second;
        note(key);
        return nullptr;
    }
    // the data of `key` if it holds exactly n floats
    const float* get(const std::string& key, size_t n) {
        const HostTensor* t = find(key);
        if (t && t->data.size() != n) note(key + " (wrong size)");
        return t && t->data.size() == n ? t->data.data() : nullptr;
    }
    void raw(const std::string& key, const float** slot, size_t n) {
        if (const float* v = get(key, n)) ab.put(slot, v, n);
    }
    // *bw, *bb = the bound of the 1x1 / conv `name` (weight [M][K]), a hair above in float so that rounding cannot undercut it
    void bound(const std::string& name, int M, int K, float* bw, float* bb) {
        const float* w = get(name + ".weight", (size_t)M * K);
        const float* b = get(name + ".bias", M);
        if (!w || !b) return;
        const RowL1 r = row_l1(w, b, M, K);
        *bw = (float)(r.w * 1.0001);
        *bb = (float)(r.b * 1.0001);
    }

    // Stack one or more conv weights [cout_i][cin][taps] along cout into the host staging layout At[k][m], k = ci*taps + tap
    // (zero-padded to Kpad x Mpad) and the bias row [Mpad].
    bool stage(const std::vector<std::string>& names, PackedW* pw, int cin, int taps, std::vector<float>* At, std::vector<float>* bias, int* group_rows) {
        int M = 0;
        std::vector<const HostTensor*> ws, bs;
        for (auto& n : names) {
            const HostTensor* w = find(n + ".weight");
            const HostTensor* b = find(n + ".bias");
            if (!w || !b) return false;
            if (w->shape.size() != 3 || w->shape[1] != cin || w->shape[2] != taps ||
                (int64_t)b->data.size() != w->shape[0]) {
                note(n + " (unexpected shape)");
                return false;
            }
            ws.push_back(w);
            bs.push_back(b);
            M += (int)w->shape[0];
        }
        pw->M = M;
        pw->K = cin * taps;
        pw->cin = cin;
        pw->taps = taps;
        pw->Mpad = pad_m(M);
        pw->Kpad = (pw->K + 15) / 16 * 16;
        At->assign((size_t)pw->Kpad * pw->Mpad, 0.f);
        bias->assign(pw->Mpad, 0.f);
        int m0 = 0;
        for (size_t i = 0; i < ws.size(); ++i) {
            int cout = (int)ws[i]->shape[0];
            for (int m = 0; m < cout; ++m) {
                (*bias)[m0 + m] = bs[i]->data[m];
                for (int k = 0; k < pw->K; ++k) (*At)[(size_t)k * pw->Mpad + m0 + m] = ws[i]->data[(size_t)m * pw->K + k];
            }
            m0 += cout;
        }
        bool equal_groups = ws.size() > 1;
        for (auto* w : ws) equal_groups = equal_groups && w->shape[0] == ws[0]->shape[0];
        *group_rows = equal_groups ? (int)ws[0]->shape[0] : 0;
        return true;
    }
    // image geometry: group_rows > 0 = the M rows are `M / group_rows` stacked groups (FiLM scale ; shift), each padded to whole 32-row tiles
    static int image_mt(const PackedW* pw, int group_rows) {
        const int gp = group_rows > 0 ? (group_rows + 31) / 32 * 32 : 0;
        return group_rows > 0 ? (pw->M / group_rows) * gp / 32 : pw->Mpad / 32;
    }
    static int image_row(const PackedW* pw, int group_rows, int m) {      // staged row of image row m (pw->M = a padding row)
        if (group_rows <= 0) return m < pw->M ? m : pw->M;
        const int gp = (group_rows + 31) / 32 * 32, g = m / gp, mi = m - g * gp;
        return mi < group_rows ? g * group_rows + mi : pw->M;
    }
    std::vector<float> mt_amax(const PackedW* pw, const std::vector<float>& At, int group_rows) {
        const int MT = image_mt(pw, group_rows);
        std::vector<float> amax(MT, 0.f);
        for (int mt = 0; mt < MT; ++mt)
            for (int r = 0; r < 32; ++r) {
                const int m = image_row(pw, group_rows, mt * 32 + r);
                if (m >= pw->M) continue;
                for (int k = 0; k < pw->K; ++k) amax[mt] = std::max(amax[mt], std::fabs(At[(size_t)k * pw->Mpad + m]));
            }
        return amax;
    }
    void conv(const std::vector<std::string>& names, PackedW* pw, int cin, int taps) {
        std::vector<float> At, bias;
        int group_rows = 0;
        if (!stage(names, pw, cin, taps, &At, &bias, &group_rows)) return;
        // only the split image goes to the device: `At` is the host-side staging layout it is built from
        ab.put(&pw->bias, bias);
        std::vector<float> sc = mt_amax(pw, At, group_rows);
        for (auto& v : sc) v = pow2_scale(v);
        a6(pw, At, group_rows, sc);
    }
    // two convs whose results are accumulated into ONE tile (Downsample: c3(h2) + down_res(xi)): the same per-m-tile scales for both
    void conv_joint(const std::string& na, PackedW* pa, int cin_a, int taps_a, const std::string& nb, PackedW* pb, int cin_b, int taps_b) {
        std::vector<float> Aa, ba, Ab, bb;
        int ga = 0, gb = 0;
        if (!stage({na}, pa, cin_a, taps_a, &Aa, &ba, &ga) || !stage({nb}, pb, cin_b, taps_b, &Ab, &bb, &gb)) return;
        if (pa->Mpad != pb->Mpad) return note(na + " / " + nb + " (row counts differ)");
        ab.put(&pa->bias, ba);
        ab.put(&pb->bias, bb);
        std::vector<float> sa = mt_amax(pa, Aa, 0), sb = mt_amax(pb, Ab, 0);
        for (size_t i = 0; i < sa.size(); ++i) sa[i] = pow2_scale(std::max(sa[i], sb[i]));
        const size_t off_a = a6(pa, Aa, 0, sa);
        a6(pb, Ab, 0, sa);
        ab.fix.push_back({&pb->wjoint, off_a});      // resolves to pa->A6: the launch checks that the pair was packed together
    }
    // two-part fp16 image of At for conv3s.h: [step = slab*taps + tap][m-tile][part][lane][8 fp16],
    // lane -> row m = 32*mt + (lane & 31), channel ci = 16*slab + 8*(lane >> 5) + j.  Returns the image's arena offset.
    size_t a6(PackedW* pw, const std::vector<float>& At, int group_rows, const std::vector<float>& scale) {
        const int taps = pw->taps, cin = pw->cin, nslab = ((cin + 15) / 16 + 5) / 6 * 6;   // zero slabs up to a multiple of 6: any slab depth divides
        const int MT = image_mt(pw, group_rows);
        std::vector<float> img((size_t)nslab * taps * MT * 2 * 256, 0.f);
        uint16_t* o = reinterpret_cast<uint16_t*>(img.data());
        for (int s = 0; s < nslab; ++s)
            for (int tap = 0; tap < taps; ++tap)
                for (int mt = 0; mt < MT; ++mt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int ci = s * 16 + 8 * (lane >> 5) + j, m = image_row(pw, group_rows, mt * 32 + (lane & 31));
                            const float w = (ci < cin && m < pw->M) ? At[(size_t)(ci * taps + tap) * pw->Mpad + m] : 0.f;
                            const size_t base = (((size_t)(s * taps + tap) * MT + mt) * 2 * 64 + lane) * 8 + j;
                            split2(w, scale[mt], &o[base], &o[base + 512]);
                        }
        pw->MT6 = MT;
        pw->S6 = nslab;
        const size_t off = ab.put(&pw->A6, img);
        ab.put(&pw->wscale, scale);
        host_wscale[pw] = scale;
        return off;
    }
    // conv (k3) + FiLM (two 1x1s) of one Upsample half for film_s2.h.  Image: [96-row block][16-channel slab][30 pieces][lane][8 fp16],
    // piece q < 18: conv tap q / 6, m-tile (q % 6) / 2 of the block, part q % 2; q >= 18: to_scale (q < 24) / to_shift, m-tile, part.
    // Lane order as in a6 (row = lane & 31, channel = 16 slab + 8 (lane >> 5) + j).  This kernel adds all three part products into ONE
    // accumulator, so the second part is the UNSCALED fp16 residual and every m-tile is normalised to |max| in [2^13, 2^14): the
    // residual's absolute fp16 resolution (2^-24, subnormals kept) is then 2^-37 of the tile's largest weight.  C is a multiple of 96.
    void film_u(FilmU* fu, const std::string& conv_name, const std::string& film, int C, const std::string& first_conv) {
        const size_t CC = (size_t)C * C;
        const float* w = get(conv_name + ".weight", 3 * CC);
        const float* b = get(conv_name + ".bias", C);
        const float* wsc = get(film + ".to_scale.weight", CC);
        const float* bsc = get(film + ".to_scale.bias", C);
        const float* wsh = get(film + ".to_shift.weight", CC);
        const float* bsh = get(film + ".to_shift.bias", C);
        if (!w || !b || !wsc || !bsc || !wsh || !bsh) return;
        const int MT = C / 32, nslab = C / 16, mblocks = C / 96;
        auto tile_scale = [&](const float* wt, int per_row, int mt) { return pow2_scale(amax(wt + (size_t)mt * 32 * per_row, (size_t)32 * per_row)) * (1.f / 8192.f); };
        std::vector<float> tab((size_t)6 * C);
        auto row = [&](int r) { return &tab[(size_t)r * C]; };
        float *scale_conv = row(FilmU::TAB_SCALE), *scale_sc = row(FilmU::TAB_SSC), *scale_sh = row(FilmU::TAB_SSH);
        std::copy(b, b + C, row(FilmU::TAB_BIAS));
        std::copy(bsc, bsc + C, row(FilmU::TAB_BSC));
        std::copy(bsh, bsh + C, row(FilmU::TAB_BSH));
        for (int mt = 0; mt < MT; ++mt) {
            std::fill_n(scale_conv + 32 * mt, 32, tile_scale(w, 3 * C, mt));
            std::fill_n(scale_sc + 32 * mt, 32, tile_scale(wsc, C, mt));
            std::fill_n(scale_sh + 32 * mt, 32, tile_scale(wsh, C, mt));
        }
        std::vector<float> img((size_t)mblocks * nslab * 30 * 64 * 4, 0.f);
        uint16_t* o = reinterpret_cast<uint16_t*>(img.data());
        for (int mb = 0; mb < mblocks; ++mb)
            for (int s = 0; s < nslab; ++s)
                for (int q = 0; q < 30; ++q) {
                    const bool conv = q < 18;
                    const int qq = conv ? q : q - 18, grp = qq / 6, mi = (qq % 6) / 2, part = qq % 2, mt = mb * 3 + mi;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int m = mt * 32 + (lane & 31), ci = s * 16 + 8 * (lane >> 5) + j;
                            float x;
                            if (conv) x = w[((size_t)m * C + ci) * 3 + grp] / scale_conv[m];
                            else if (grp == 0) x = wsc[(size_t)m * C + ci] / scale_sc[m];
                            else x = wsh[(size_t)m * C + ci] / scale_sh[m];
                            const uint16_t h1 = f16_bits(x);
                            o[((((size_t)mb * nslab + s) * 30 + q) * 64 + lane) * 8 + j] = part == 0 ? h1 : f16_bits(x - f16_value(h1));
                        }
                }
        // the bound the half's first conv normalises its pre-split output by (conv_s2.h PRE)
        bound(first_conv, C, 3 * C, &fu->hb_w, &fu->hb_b);
        fu->C = C;
        ab.put(&fu->img, img);
        ab.put(&fu->tab, tab);
    }
    // Weight blob of one half of the fused ups.4 kernel (filter_up24s.hip), layout Up24sBlob: 28 pieces in the K-unit layout (put_k24)
    //   [conv a: 5 steps][2 parts] [conv b: 5 steps][2 parts] [FiLM: 2 steps][to_scale, to_shift][2 parts]
    // then the biases, the folded output conv, the four weight scales and the bound of the block's on-chip intermediate (see the kernel).
    // Second half: Upsample.c5 (1x1, decoder.py:171,189) and FilterNet.output_layer (k7, decoder.py:220,233) have nothing
    // between them, so they are one k7 conv 24 -> 1: w75[c][j] = sum_m w7[m][j] w5[m][c], b75 = b7 + sum_{m,j} w7[m][j] b5[m]
    // (replicate padding commutes with the 1x1), accumulated in double.
    void up24s_half(const float** slot, const std::string& ca, const std::string& cb, const std::string& film, const std::string& c5,
                    const std::string& out7) {
        using L = Up24sBlob;
        constexpr int C = 24;
        const float* wa = get(ca + ".weight", C * C * 3);
        const float* ba = get(ca + ".bias", C);
        const float* wb = get(cb + ".weight", C * C * 3);
        const float* bb = get(cb + ".bias", C);
        const float* wsc = get(film + ".to_scale.weight", C * C);
        const float* bsc = get(film + ".to_scale.bias", C);
        const float* wsh = get(film + ".to_shift.weight", C * C);
        const float* bsh = get(film + ".to_shift.bias", C);
        if (!wa || !ba || !wb || !bb || !wsc || !bsc || !wsh || !bsh) return;
        std::vector<float> img(L::PIECES * 256 + L::FLOATS, 0.f);
        float* fl = img.data() + L::PIECES * 256;
        fl[L::SA] = pow2_scale(amax(wa, C * C * 3));
        fl[L::SB] = pow2_scale(amax(wb, C * C * 3));
        fl[L::SSC] = pow2_scale(amax(wsc, C * C));
        fl[L::SSH] = pow2_scale(amax(wsh, C * C));
        put_k24(img, 0, 2, wa, C, C, 3, &fl[L::SA]);
        put_k24(img, 10, 2, wb, C, C, 3, &fl[L::SB]);
        put_k24(img, 20, 4, wsc, C, C, 1, &fl[L::SSC]);
        put_k24(img, 22, 4, wsh, C, C, 1, &fl[L::SSH]);
        std::copy(ba, ba + C, fl + L::BA);
        std::copy(bb, bb + C, fl + L::BB);
        std::copy(bsc, bsc + C, fl + L::BSC);
        std::copy(bsh, bsh + C, fl + L::BSH);
        const RowL1 r = row_l1(wa, ba, C, C * 3);
        fl[L::L1A] = (float)(r.w * 1.0000002);      // rounded up: it is a bound
        fl[L::BMA] = (float)r.b;
        if (!c5.empty()) {
            const float* w5 = get(c5 + ".weight", C * C);
            const float* b5 = get(c5 + ".bias", C);
            const float* w7 = get(out7 + ".weight", C * 7);
            const float* b7 = get(out7 + ".bias", 1);
            if (!w5 || !b5 || !w7 || !b7) return;
            double bias = b7[0];
            for (int c = 0; c < C; ++c)
                for (int j = 0; j < 7; ++j) {
                    double acc = 0.0;
                    for (int m = 0; m < C; ++m) acc += (double)w7[(size_t)m * 7 + j] * (double)w5[(size_t)m * C + c];
                    fl[L::W75 + c * 7 + j] = (float)acc;
                }
            for (int m = 0; m < C; ++m)
                for (int j = 0; j < 7; ++j) bias += (double)w7[(size_t)m * 7 + j] * (double)b5[m];
            fl[L::B75] = (float)bias;
        }
        ab.put(slot, img);
    }
    // Weight blob of the downs.0 kernel (filter_up24s.hip), layout Down0sBlob: the 17 -> 24 k3 conv in the K-unit layout of a 24-channel
    // conv (input channels 17..23 zero).  *bound_w, *bound_b: the bound of its output.
    void down0s(const float** slot, const std::string& name, float* bound_w, float* bound_b) {
        using L = Down0sBlob;
        constexpr int C = 24, CI = 17;
        const float* w = get(name + ".weight", C * CI * 3);
        const float* b = get(name + ".bias", C);
        if (!w || !b) return;
        std::vector<float> img(L::PIECES * 256 + L::FLOATS, 0.f);
        float* fl = img.data() + L::PIECES * 256;
        fl[L::SCALE] = pow2_scale(amax(w, C * CI * 3));
        put_k24(img, 0, 2, w, C, CI, 3, &fl[L::SCALE]);
        std::copy(b, b + C, fl + L::BIAS);
        // |out| <= l1max |x|max + bmax (rounded up a little: the bound must hold for the fp32-rounded sums too): the scale of the pre-split planes
        const RowL1 r = row_l1(w, b, C, CI * 3);
        fl[L::BW] = *bound_w = (float)(r.w * 1.0001);
        fl[L::BB] = *bound_b = (float)r.b * 1.0001f;
        ab.put(slot, img);
    }
    // Weight blob of one 24-input-channel k3 conv for down24f_kernel (filter_up24s.hip), layout Conv24sBlob: pieces [step][m-tile][part]
    // in the K-unit layout, bias + `extra_bias`.  M = 24 (one m-tile) or 48 (two).  `joint`: take the scales of this already packed image
    // instead of the weight's own (c3 of the 24-channel Downsample block is accumulated with down_res into one tile: conv_joint).
    void conv24s(const float** slot, const std::string& name, int M, const std::string& extra_bias = "", const PackedW* joint = nullptr) {
        constexpr int CI = 24;
        const int MT = (M + 31) / 32;
        const float* w = get(name + ".weight", (size_t)M * CI * 3);
        const float* b = get(name + ".bias", M);
        const float* eb = extra_bias.empty() ? nullptr : get(extra_bias, M);
        if (!w || !b || (!extra_bias.empty() && !eb)) return;
        std::vector<float> img((size_t)K24_PIECES * MT * 256 + Conv24sBlob::FLOATS, 0.f);
        float* fl = img.data() + (size_t)K24_PIECES * MT * 256;
        float* sc = fl + Conv24sBlob::SCALE;
        if (joint) {
            auto it = host_wscale.find(joint);
            if (it == host_wscale.end() || (int)it->second.size() != MT) return note(name + " (its joint image is not packed yet)");
            std::copy(it->second.begin(), it->second.end(), sc);
        } else {
            for (int mt = 0; mt < MT; ++mt) sc[mt] = pow2_scale(amax(w + (size_t)32 * mt * CI * 3, (size_t)(std::min(M, 32 * mt + 32) - 32 * mt) * CI * 3));
        }
        put_k24(img, 0, 2 * MT, w, M, CI, 3, sc);
        for (int m = 0; m < M; ++m) fl[Conv24sBlob::BIAS + m] = b[m] + (eb ? eb[m] : 0.f);
        ab.put(slot, img);
    }
    void convnext(const std::string& p, ConvNeXtW* w, int C, int dil) {
        w->C = C;
        w->dilation = dil;
        raw(p + ".c1.weight", &w->dw_w, (size_t)C * 7);
        raw(p + ".c1.bias", &w->dw_b, C);
        const float* g = get(p + ".norm.gamma", C);
        const float* bt = get(p + ".norm.beta", C);
        if (g) ab.put(&w->ln_g, g, C);
        if (bt) ab.put(&w->ln_b, bt, C);
        if (g && bt) {   // |LayerNorm output| <= sqrt(C - 1) max|gamma| + max|beta| whatever the data (a normalised column has |x_hat| <= sqrt(C - 1))
            const RowL1 r = row_l1(g, bt, C, 1);
            w->ln_bound = std::sqrt((float)C) * (float)r.w + (float)r.b;
        }
        conv({p + ".c2"}, &w->c2, C, 1);
        raw(p + ".grn.gamma", &w->grn_g, 2 * C);
        raw(p + ".grn.beta", &w->grn_b, 2 * C);
        conv({p + ".c3"}, &w->c3, 2 * C, 1);
        const float* w3 = get(p + ".c3.weight", (size_t)C * 2 * C);
        const float* b3 = get(p + ".c3.bias", C);
        const float* gb = get(p + ".grn.beta", 2 * C);
        if (w3 && b3 && gb) {
            std::vector<float> fb(w->c3.Mpad, 0.f);
            for (int m = 0; m < C; ++m) {
                double acc = b3[m];
                for (int k = 0; k < 2 * C; ++k) acc += (double)w3[(size_t)m * 2 * C + k] * (double)gb[k];
                fb[m] = (float)acc;
            }
            ab.put(&w->c3_bias_grn, fb);
        }
    }
};

}  // namespace

// Tables of the wave-level 1920-point FFTs (fft.hip), computed in fp64: (cos, sin)(2 pi j / 960), (cos, sin)(2 pi k / 1920),
// periodic Hann window.  Behind them the tables of the streams' spectral suppressor (denoise.hip), fp64-made too: the square-root Hann
// window of its 640-sample frames, (cos, sin)(2 pi j / 320) and (cos, sin)(2 pi k / 640).
void pack_constants(tvc_ctx* ctx, ArenaBuilder* ab) {
    const int N = kNfft;
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<float> t960(2 * 960), t1920(2 * 961 + 2), hann(N);
    for (int j = 0; j < 960; ++j) {
        t960[2 * j] = (float)std::cos(two_pi * j / 960.0);
        t960[2 * j + 1] = (float)std::sin(two_pi * j / 960.0);
    }
    for (int k = 0; k <= 960; ++k) {
        t1920[2 * k] = (float)std::cos(two_pi * k / 1920.0);
        t1920[2 * k + 1] = (float)std::sin(two_pi * k / 1920.0);
    }
    for (int n = 0; n < N; ++n) hann[n] = (float)(0.5 - 0.5 * std::cos(two_pi * n / N));
    ab->put(&ctx->fft_tw960, t960);
    ab->put(&ctx->fft_tw1920, t1920);
    ab->put(&ctx->fft_hann, hann);
    ab->put(&ctx->sola_part, std::vector<float>(kSolaPartFloats, 0.f));   // device scratch, not a table (sola.hip)
    const int F = kDenoiseFrame;
    std::vector<float> win(F), t320(2 * (F / 2)), t640(2 * (F / 2 + 1));
    for (int n = 0; n < F; ++n) win[n] = (float)std::sqrt(0.5 - 0.5 * std::cos(two_pi * n / F));
    for (int j = 0; j < F / 2; ++j) {
        t320[2 * j] = (float)std::cos(two_pi * j / (F / 2));
        t320[2 * j + 1] = (float)std::sin(two_pi * j / (F / 2));
    }
    for (int k = 0; k <= F / 2; ++k) {
        t640[2 * k] = (float)std::cos(two_pi * k / F);
        t640[2 * k + 1] = (float)std::sin(two_pi * k / F);
    }
    ab->put(&ctx->dn_win, win);
    ab->put(&ctx->dn_tw320, t320);
    ab->put(&ctx->dn_tw640, t640);
}

void pack_checkpoint(tvc_ctx* ctx, ArenaBuilder* ab, std::string* missing_enc, std::string* missing_dec) {
    Packer pk{ctx, *ab};
    if (ctx->pitch_table.size() == (size_t)kPitchClasses)
        ab->put(&ctx->pitch_freq, ctx->pitch_table);
    else
        pk.missing = "pitch table (tvc_set_pitch_table)";

    // encoder (encoder.py:75-116): both estimators read the same spectrogram -> stacked input 1x1
    pk.conv({"ssl_feature_estimator.input_layer", "pitch_estimator.input_layer"}, &ctx->enc_in, kBins, 1);
    pk.raw("ssl_feature_estimator.norm.gamma", &ctx->ssl_ln_g, kSslCh);
    pk.raw("ssl_feature_estimator.norm.beta", &ctx->ssl_ln_b, kSslCh);
    pk.raw("pitch_estimator.norm.gamma", &ctx->pit_ln_g, kPitchCh);
    pk.raw("pitch_estimator.norm.beta", &ctx->pit_ln_b, kPitchCh);
    static const int ssl_dil[6] = {1, 3, 9, 1, 1, 1};
    for (int i = 0; i < 6; ++i)
        pk.convnext("ssl_feature_estimator.mid_layers." + std::to_string(i), &ctx->ssl_mid[i], kSslCh, ssl_dil[i]);
    for (int i = 0; i < 4; ++i)
        pk.convnext("pitch_estimator.mid_layers." + std::to_string(i), &ctx->pit_mid[i], kPitchCh, 1);
    pk.conv({"ssl_feature_estimator.output_layer"}, &ctx->ssl_out, kSslCh, 1);
    pk.conv({"pitch_estimator.output_layer"}, &ctx->pit_out, kPitchCh, 1);
    *missing_enc = pk.missing;
    pk.missing.clear();

    // source net (decoder.py:102-134)
    pk.conv({"source_net.content_in"}, &ctx->src_content_in, kSslDim, 1);
    pk.raw("source_net.energy_in.weight", &ctx->src_e_w, kSrcCh);
    pk.raw("source_net.energy_in.bias", &ctx->src_e_b, kSrcCh);
    pk.raw("source_net.f0_in.weight", &ctx->src_f_w, kSrcCh);
    pk.raw("source_net.f0_in.bias", &ctx->src_f_b, kSrcCh);
    for (int i = 0; i < 3; ++i)
        pk.convnext("source_net.mid_layers." + std::to_string(i), &ctx->src_mid[i], kSrcCh, 1);
    pk.conv({"source_net.to_amps"}, &ctx->src_to_amps, kSrcCh, 1);
    pk.conv({"source_net.to_kernel"}, &ctx->src_to_kernel, kSrcCh, 1);

    // filter net (decoder.py:193-233); the images of each level are those its launches read (decoder.hip run_filter)
    static const int ch[5] = {384, 192, 96, 48, 24};
    static const int fac[5] = {2, 3, 4, 4, 5};
    pk.conv({"filter_net.content_in"}, &ctx->flt_content_in, kSslDim, 1);
    pk.raw("filter_net.f0_in.weight", &ctx->flt_f_w, ch[0]);
    pk.raw("filter_net.f0_in.bias", &ctx->flt_f_b, ch[0]);
    // analytic |max| bounds of 1x1 outputs: the slot of a tensor an epilogue functor finishes comes from its input's slot instead of a
    // pass over the tensor
    pk.bound("filter_net.content_in", ch[0], kSslDim, &ctx->flt_in_bw, &ctx->flt_in_bb);
    {   // + f0_in(log(relu(f0) + 1e-6)): |log| < 89 for every finite fp32 f0 (f0_in is a 1x1 from one channel: its row sums are max |w|)
        const float* fw = pk.get("filter_net.f0_in.weight", ch[0]);
        const float* fb = pk.get("filter_net.f0_in.bias", ch[0]);
        if (fw && fb) {
            const RowL1 r = row_l1(fw, fb, ch[0], 1);
            ctx->flt_in_bb += (float)((r.w * 89.0 + r.b) * 1.0001);
        }
    }
    pk.down0s(&ctx->flt_down0s, "filter_net.downs.0", &ctx->down0_bw, &ctx->down0_bb);
    for (int i = 1; i <= 4; ++i) {
        DownW& d = ctx->downs[i - 1];
        d.cin = ch[5 - i];
        d.cout = ch[4 - i];
        d.factor = fac[5 - i];
        std::string p = "filter_net.downs." + std::to_string(i);
        pk.conv_joint(p + ".c3", &d.c3, d.cin, 3, p + ".down_res", &d.res, d.cin, 1);      // c3(h2) + down_res(xi) land in one tile: joint scales
        if (d.cin == 24) {   // down24f_kernel: its three blobs, down_res's image, and the bounds of its on-chip intermediates
            pk.conv24s(&d.s24c1, p + ".c1", 24);
            pk.conv24s(&d.s24c2, p + ".c2", 24);
            pk.conv24s(&d.s24c3r, p + ".c3", 48, p + ".down_res.bias", &d.c3);
            pk.bound(p + ".c1", 24, 72, &d.b1_w, &d.b1_b);
            pk.bound(p + ".c2", 24, 72, &d.b2_w, &d.b2_b);
            continue;
        }
        pk.conv({p + ".c1"}, &d.c1, d.cin, 3);
        pk.conv({p + ".c2"}, &d.c2, d.cin, 3);
        // c3.bias + down_res.bias for the launches that accumulate both convs into one tile
        const float* b3 = pk.get(p + ".c3.bias", d.cout);
        const float* br = pk.get(p + ".down_res.bias", d.cout);
        if (b3 && br) {
            std::vector<float> sum(d.c3.Mpad, 0.f);
            for (int m = 0; m < d.cout; ++m) sum[m] = b3[m] + br[m];
            ab->put(&d.c3res_bias, sum);
        }
    }
    for (int i = 0; i < 5; ++i) {
        UpW& u = ctx->ups[i];
        u.cin = ch[i];
        u.cout = i < 4 ? ch[i + 1] : ch[4];
        u.factor = fac[i];
        std::string p = "filter_net.ups." + std::to_string(i);
        if (u.cin == 24) {   // the fused block (run_up24_split): two blobs, which between them read every tensor of the level
            pk.up24s_half(&u.s24a, p + ".c1", p + ".c2", p + ".film1", "", "");
            pk.up24s_half(&u.s24b, p + ".c3", p + ".c4", p + ".film2", p + ".c5", "filter_net.output_layer");
            continue;
        }
        pk.conv({p + ".c1"}, &u.c1, u.cin, 3);
        pk.conv({p + ".c2"}, &u.c2, u.cin, 3);
        pk.conv({p + ".c3"}, &u.c3, u.cin, 3);
        pk.conv({p + ".c4"}, &u.c4, u.cin, 3);
        pk.conv({p + ".c5"}, &u.c5, u.cin, 1);
        pk.bound(p + ".c5", u.cout, u.cin, &u.c5_bw, &u.c5_bb);
        pk.conv({p + ".film1.to_scale", p + ".film1.to_shift"}, &u.film1, u.cin, 1);
        pk.conv({p + ".film2.to_scale", p + ".film2.to_shift"}, &u.film2, u.cin, 1);
        if (u.cin >= 96) {
            pk.film_u(&u.fu1, p + ".c2", p + ".film1", u.cin, p + ".c1");
            pk.film_u(&u.fu2, p + ".c4", p + ".film2", u.cin, p + ".c3");
        }
    }
    *missing_dec = pk.missing;
}

}  // namespace tvc

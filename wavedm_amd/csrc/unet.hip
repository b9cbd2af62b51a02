// Whole-UNet executor: builds the layer list of the reference's DiffusionUNet (models/unet.py:197-307) from the
// config, owns the layout of the single packed-weight buffer, and runs forward (unet.py:346-395) as a fixed sequence
// of fused-kernel launches on one stream.  Parameter names / shapes are exactly the reference's state_dict keys.
#include <string.h>

#include <map>
#include <mutex>
#include <string>

#include "common.h"

namespace wdm {
const char* get_error();
}
using namespace wdm;

namespace {

enum ParamKind { PK_CONV, PK_F32 };

// where a parameter of the layout lands in the packed buffer (wdm_unet::slots, parallel to the layout's parameter list)
struct ParamSlot {
    ParamKind kind = PK_F32;
    size_t off = 0;       // byte offset of the destination matrix / vector in the packed buffer
    int rows_total = 0;   // PK_CONV: rows of the destination matrix (fused qk: 2C)
    int row_off = 0;      // PK_CONV: first destination row;  PK_F32: element offset inside the destination vector
    bool zero_tail = true;   // PK_CONV: this slot also zero-fills the padding rows behind it
    int cin_dst = 0;         // PK_CONV: row length of the destination when it is padded beyond shape[1] (conv_in), else 0
    size_t sm_off = 0;       // PK_CONV of a bf16 3x3 conv: second destination, the slab-major copy (k_pack_conv_sm); 0 = none
    size_t up4_off = 0;      // PK_CONV of an Upsample conv (bf16): second destination, the 16 sub-pixel taps (k_pack_up4); 0 = none
    bool loaded = false;
    int fold = -1, fold_role = -1;   // tensor of an AttnBlock whose folded operands are rebuilt when it is loaded (16-bit modes): index into wdm_unet::folds, FR_* role
};
inline ParamSlot slot_at(ParamKind kind, size_t off, int rows_total = 0, int row_off = 0) { ParamSlot s; s.kind = kind; s.off = off; s.rows_total = rows_total; s.row_off = row_off; return s; }

// a conv's operands in the packed buffer (wdm_unet::convd, parallel to the layout's conv list; q and k of an AttnBlock share the fused [2C][C] matrix)
struct ConvD { size_t w_off, b_off; int cin, cout, k, rows_pad; size_t up4_off, sm_off; };
// folded AttnBlock operands (common.h: k_attn_fold): the fp32 originals of the four matrices are kept ([Wq | Wk | Wv | Wp] at stage_off) so that any one tensor can be
// reloaded; the biases' fp32 copies are the ones the unfolded convs use
enum { FR_QW = 0, FR_KW, FR_VW, FR_PW, FR_QB, FR_VB, FR_PB, FR_N };
struct FoldD { int c; size_t stage_off; ConvD qk, v, proj, qf, pf; int slot[FR_N]; };
// a layer output of the forward that a caller can have copied out (wdm_unet_forward_taps), in executor order.  in0: the tap the layer reads (-1: the network's input);
// in1: an up block's skip, the second half of its concat (else -1)
struct TapD { std::string name; int C, H, W, kind, in0, in1; };

}  // namespace

struct wdm_unet {
    using Conv = UNetLayout::Conv;
    using Norm = UNetLayout::Norm;
    using Res = UNetLayout::Res;
    using Attn = UNetLayout::Attn;
    wdm_handle* h;
    wdm_unet_config cfg;
    UNetLayout L;                   // the network; L.params also lists the temb_proj tail (weight, bias per layer)
    std::vector<ParamSlot> slots;   // per parameter
    std::vector<ConvD> convd;       // per conv
    std::map<std::string, int> index;
    size_t packed_bytes = 0;
    size_t range_flag_off = 0;      // WDM_F16 only
    std::vector<FoldD> folds;       // 16-bit modes: one per AttnBlock
    size_t fold_tmp_floats = 0, fold_tmp_off = 0;
    char* packed = nullptr;
    bool all_loaded = false;
    size_t temb_w_off = 0, temb_b_off = 0;
    std::vector<TapD> taps;         // wdm_unet_tap_info: one per launch sequence of forward() that leaves a layer's output

    // ---- the packed buffer, laid out in one pass over the layout (the order of the take() calls IS the buffer's format: it is broadcast between ranks)
    size_t take(size_t bytes) { size_t o = packed_bytes; packed_bytes = align_up(packed_bytes + bytes, 256); return o; }
    void place_f32(int pi) { slots[pi] = slot_at(PK_F32, take((size_t)L.params[pi].numel() * 4)); }
    // cin_pad > cin: the kernels' K dimension is padded with zero columns (conv_in of a model whose input width is not a multiple of 32)
    // s1: the conv gets the slab-major weight copy: stride-1 convs, and since round 5 the Downsample convs of the 16-bit modes (conv_s2_kernel.h); Upsample convs
    // never read theirs (their sub-pixel taps are slab-major themselves: k_pack_up4): less to pack after every trainer sync, a smaller weight broadcast
    ConvD& place_conv(const Conv& c, int cin_pad = 0, bool s1 = true) {
        ConvD d{};
        if (cin_pad <= 0) cin_pad = c.cin;
        d.cin = cin_pad; d.cout = c.cout; d.k = c.k; d.rows_pad = conv_rows_pad(c.cout);
        d.w_off = take(conv_packed_bytes(cin_pad, c.cout, c.k, cfg.dtype));
        d.b_off = take((size_t)c.cout * 4);
        slots[c.w] = slot_at(PK_CONV, d.w_off, d.rows_pad);
        slots[c.w].cin_dst = cin_pad != c.cin ? cin_pad : 0;
        if (s1 && cin_pad == c.cin && conv_sm_eligible(cfg.dtype, c.k, c.cin)) slots[c.w].sm_off = d.sm_off = take(conv_packed_bytes(c.cin, c.cout, c.k, cfg.dtype));
        slots[c.b] = slot_at(PK_F32, d.b_off);
        return convd[c.idx] = d;
    }
    void place_norm(const Norm& n) { place_f32(n.g); place_f32(n.b); }
    void place_res(const Res& r) {
        place_norm(r.n1); place_conv(r.c1);
        place_norm(r.n2); place_conv(r.c2);
        if (r.has_nin) place_conv(r.nin);
    }
    void place_attn(const Attn& a) {
        const int c = a.c;
        place_norm(a.n);
        // q and k are fused into one [2C][C] matrix: one pass over the normalised input produces both
        ConvD qk{};
        qk.cin = c; qk.cout = 2 * c; qk.k = 1; qk.rows_pad = conv_rows_pad(2 * c);
        qk.w_off = take(conv_packed_bytes(c, 2 * c, 1, cfg.dtype));
        qk.b_off = take((size_t)2 * c * 4);
        slots[a.q.w] = slot_at(PK_CONV, qk.w_off, qk.rows_pad, 0);
        slots[a.q.w].zero_tail = false;   // the k slot below owns the rows behind q
        slots[a.q.b] = slot_at(PK_F32, qk.b_off, 0, 0);
        slots[a.k.w] = slot_at(PK_CONV, qk.w_off, qk.rows_pad, c);
        slots[a.k.b] = slot_at(PK_F32, qk.b_off, 0, c);
        convd[a.q.idx] = convd[a.k.idx] = qk;
        place_conv(a.v);
        place_conv(a.proj);
        if (is_h16(cfg.dtype)) {
            // the folded operands the fused core runs on (blocks.hip: run_attn), rebuilt by wdm_unet_load_param whenever one of the seven tensors behind them arrives
            FoldD f{};
            f.c = c;
            auto plain = [&](ConvD& d) { d = ConvD{}; d.cin = c; d.cout = c; d.k = 1; d.rows_pad = conv_rows_pad(c); d.w_off = take(conv_packed_bytes(c, c, 1, cfg.dtype)); d.b_off = take((size_t)c * 4);
                                        if (c % 32 == 0) d.sm_off = take(conv_packed_bytes(c, c, 1, cfg.dtype)); };      // + the slab-major copy the fused core streams (attn_fused_kernel.h)
            plain(f.qf); plain(f.pf);
            f.stage_off = take((size_t)4 * c * c * 4);
            f.qk = qk; f.v = convd[a.v.idx]; f.proj = convd[a.proj.idx];
            const int role_slot[FR_N] = {a.q.w, a.k.w, a.v.w, a.proj.w, a.q.b, a.v.b, a.proj.b};
            for (int r = 0; r < FR_N; ++r) {
                f.slot[r] = role_slot[r];
                slots[f.slot[r]].fold = (int)folds.size();
                slots[f.slot[r]].fold_role = r;
            }
            fold_tmp_floats = std::max(fold_tmp_floats, (size_t)c * c);
            folds.push_back(f);
        }
    }

    int build();
    ConvW cw(const ConvD& d) const { ConvW w; w.w = packed + d.w_off; w.w_up4 = d.up4_off ? packed + d.up4_off : nullptr; w.w_sm = d.sm_off ? packed + d.sm_off : nullptr; w.b = (const float*)(packed + d.b_off); w.cin = d.cin; w.cout = d.cout; w.k = d.k; w.rows_pad = d.rows_pad; return w; }
    ConvW cw(const Conv& c) const { return cw(convd[c.idx]); }
    NormW nw(const Norm& d) const { NormW n; n.g = (const float*)(packed + slots[d.g].off); n.b = (const float*)(packed + slots[d.b].off); n.c = d.c; return n; }
    ResW rw(const Res& d, const float* temb_all, int n_t) const {
        ResW r;
        r.cin = d.cin; r.cout = d.cout; r.n1 = nw(d.n1); r.n2 = nw(d.n2); r.c1 = cw(d.c1); r.c2 = cw(d.c2);
        r.has_nin = d.has_nin;
        if (d.has_nin) r.nin = cw(d.nin);
        r.temb = temb_all ? temb_all + d.temb_row : nullptr;
        r.temb_ld = L.temb_rows;
        r.temb_per_image = n_t > 1;
        return r;
    }
    AttnW aw(const Attn& d) const {
        AttnW a; a.c = d.c; a.n = nw(d.n); a.qk = cw(d.q); a.v = cw(d.v); a.proj = cw(d.proj);
        const int fold = slots[d.q.w].fold;
        if (fold >= 0) { a.qf = cw(folds[fold].qf); a.pf = cw(folds[fold].pf); }
        return a;
    }

    int refold(const ParamSlot& p, const float* dev_src, hipStream_t s);
    int check_f16_range(const float* dev, int64_t n, const char* what, hipStream_t s, float limit = 65504.0f);
    int forward(Ctx& c, const void* x96, const float* t, int n_t, float* eps_out, const float* temb_pre = nullptr);
    int temb_table(Ctx& c, const float* t, int n_t, float* temb_all);
};

int wdm_unet::build() {
    const int nres = cfg.n_levels;
    L = unet_layout(cfg);
    slots.assign(L.params.size(), ParamSlot{});
    convd.assign(L.convs.size(), ConvD{});
    place_f32(L.d0w); place_f32(L.d0b); place_f32(L.d1w); place_f32(L.d1b);
    place_conv(L.conv_in, (int)align_up((size_t)cfg.in_channels, 32));
    for (int l = 0; l < nres; ++l) {
        for (auto& r : L.down_res[l]) place_res(r);
        for (auto& a : L.down_attn[l]) place_attn(a);
        if (l != nres - 1) place_conv(L.down_ds[l], 0, is_h16(cfg.dtype));      // (16-bit: conv_s2_kernel.h streams the slab-major copy)
    }
    place_res(L.mid1); place_attn(L.mid_attn); place_res(L.mid2);
    for (int l = nres - 1; l >= 0; --l) {
        for (auto& r : L.up_res[l]) place_res(r);
        for (auto& a : L.up_attn[l]) place_attn(a);
        if (l != 0) {
            const Conv& us = L.up_us[l];
            ConvD& d = place_conv(us, 0, false);
            if ((is_h16(cfg.dtype) || cfg.dtype == WDM_F32X3) && us.cin % 32 == 0 && us.cin >= 128)       // sub-pixel taps for conv_up4_kernel.h (either family), next to the 3x3 ones
                slots[us.w].up4_off = d.up4_off = take((size_t)16 * d.rows_pad * us.cin * dsize(cfg.dtype));
        }
    }
    place_norm(L.norm_out);
    place_conv(L.conv_out);

    // all temb_proj Linear layers concatenated into one [sum(cout)][temb_ch] fp32 matrix: one GEMV launch per step
    if (fold_tmp_floats) fold_tmp_off = take(fold_tmp_floats * 4);      // one C x C fp32 product of the AttnBlock folding, before it is packed
    if (cfg.dtype == WDM_F16) range_flag_off = take(256);      // device int the weight loader's fp16 range check writes (wdm_unet_load_param)
    temb_w_off = take((size_t)L.temb_rows * L.temb_ch * 4);
    temb_b_off = take((size_t)L.temb_rows * 4);
    int row = 0;
    for (auto& e : L.temb_proj) {
        L.params.push_back(L.temb_proj_weight(e)); slots.push_back(slot_at(PK_F32, temb_w_off, 0, row * L.temb_ch));
        L.params.push_back(L.temb_proj_bias(e)); slots.push_back(slot_at(PK_F32, temb_b_off, 0, row));
        row += e.cout;
    }
    for (size_t i = 0; i < L.params.size(); ++i) index[L.params[i].name] = (int)i;

    // the tap list: forward()'s order, the skip stack replayed on tap indices
    {
        const int nrb = cfg.num_res_blocks, R = cfg.resolution;
        const auto S = [](int v) { return std::to_string(v); };
        std::vector<int> hs;
        auto add = [&](const std::string& n, int C, int hw, int kind, int in0, int in1) { taps.push_back({n, C, hw, hw, kind, in0, in1}); return (int)taps.size() - 1; };
        int h = add("conv_in", cfg.ch, R, WDM_UNET_TAP_CONV_IN, -1, -1);
        hs.push_back(h);
        for (int l = 0; l < nres; ++l) {
            const std::string lv = "down." + S(l);
            for (int b = 0; b < nrb; ++b) {
                h = add(lv + ".block." + S(b), L.down_res[l][b].cout, R >> l, WDM_UNET_TAP_RESBLOCK, hs.back(), -1);
                if (!L.down_attn[l].empty()) h = add(lv + ".attn." + S(b), L.down_attn[l][b].c, R >> l, WDM_UNET_TAP_ATTN, h, -1);
                hs.push_back(h);
            }
            if (l != nres - 1) hs.push_back(add(lv + ".downsample", L.down_ds[l].cout, R >> (l + 1), WDM_UNET_TAP_DOWN, hs.back(), -1));
        }
        h = add("mid.block_1", L.mid1.cout, R >> (nres - 1), WDM_UNET_TAP_RESBLOCK, hs.back(), -1);
        h = add("mid.attn_1", L.mid_attn.c, R >> (nres - 1), WDM_UNET_TAP_ATTN, h, -1);
        h = add("mid.block_2", L.mid2.cout, R >> (nres - 1), WDM_UNET_TAP_RESBLOCK, h, -1);
        for (int l = nres - 1; l >= 0; --l) {
            const std::string lv = "up." + S(l);
            for (int b = 0; b <= nrb; ++b) {
                const int skip = hs.back();
                hs.pop_back();
                h = add(lv + ".block." + S(b), L.up_res[l][b].cout, R >> l, WDM_UNET_TAP_RESBLOCK, h, skip);
                if (!L.up_attn[l].empty()) h = add(lv + ".attn." + S(b), L.up_attn[l][b].c, R >> l, WDM_UNET_TAP_ATTN, h, -1);
            }
            if (l != 0) h = add(lv + ".upsample", L.up_us[l].cout, R >> (l - 1), WDM_UNET_TAP_UP, h, -1);
        }
    }
    return WDM_OK;
}

// fp16 operands: a weight outside +-65504 (or not finite) would become inf in the packed matrix -- refuse it, loudly.  The one place the weight loader waits for the
// stream (set-up path; the sampling path never does)
int wdm_unet::check_f16_range(const float* dev, int64_t n, const char* what, hipStream_t s, float limit) {
    int* flag = (int*)(packed + range_flag_off);
    int host_flag = 0;
    WDM_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
    WDM_TRY(k_flag_out_of_range(dev, n, limit, flag, s));
    WDM_HIP(hipMemcpyAsync(&host_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    WDM_HIP(hipStreamSynchronize(s));
    if (host_flag) WDM_FAIL(WDM_EINVAL, "parameter '%s': a value lies outside the fp16 range (|w| <= %.0f, finite) -- use WDM_BF16 or WDM_F32X3 for this checkpoint", what, (double)limit);
    return WDM_OK;
}

// A tensor of an AttnBlock arrived: keep the matrix's fp32 original and rebuild the folded operand it belongs to once all of that operand's tensors are there
// (q.weight, k.weight, q.bias -> qf;  v.weight, proj_out.weight, v.bias, proj_out.bias -> pf;  k.bias cancels in the softmax)
int wdm_unet::refold(const ParamSlot& p, const float* dev_src, hipStream_t s) {
    const FoldD& f = folds[p.fold];
    const size_t cc = (size_t)f.c * f.c;
    float* stage = (float*)(packed + f.stage_off);
    if (p.fold_role <= FR_PW) WDM_TRY(k_copy_f32(dev_src, stage + p.fold_role * cc, (long long)cc, s));
    const bool qk_side = p.fold_role == FR_QW || p.fold_role == FR_KW || p.fold_role == FR_QB;
    auto have = [&](std::initializer_list<int> roles) { for (int r : roles) if (!slots[f.slot[r]].loaded) return false; return true; };
    float* tmp = (float*)(packed + fold_tmp_off);
    const ConvD& dst = qk_side ? f.qf : f.pf;
    if (qk_side) {
        if (!have({FR_QW, FR_KW, FR_QB})) return WDM_OK;
        WDM_TRY(k_attn_fold(stage + FR_QW * cc, (const float*)(packed + f.qk.b_off), stage + FR_KW * cc, nullptr, nullptr, nullptr, nullptr, f.c, tmp, (float*)(packed + dst.b_off), nullptr,
                            nullptr, s));
    } else {
        if (!have({FR_VW, FR_PW, FR_VB, FR_PB})) return WDM_OK;
        WDM_TRY(k_attn_fold(nullptr, nullptr, nullptr, stage + FR_VW * cc, (const float*)(packed + f.v.b_off), stage + FR_PW * cc, (const float*)(packed + f.proj.b_off), f.c, nullptr, nullptr,
                            tmp, (float*)(packed + dst.b_off), s));
    }
    if (cfg.dtype == WDM_F16) WDM_TRY(check_f16_range(tmp, (int64_t)cc, qk_side ? "Wk^T Wq of an AttnBlock" : "Wp Wv of an AttnBlock", s));
    WDM_TRY(k_pack_conv(tmp, f.c, f.c, 1, packed + dst.w_off, dst.rows_pad, 0, 1, cfg.dtype, s));
    if (dst.sm_off) WDM_TRY(k_pack_conv_sm(tmp, f.c, f.c, packed + dst.sm_off, dst.rows_pad, s, cfg.dtype, 1));
    return WDM_OK;
}

int wdm_unet::temb_table(Ctx& c, const float* t, int n_t, float* temb_all) {
    // timestep embedding MLP + every block's temb projection: depends only on t (unet.py:10-28, 225-230, 354-357, 125)
    float *emb, *t0, *t1;
    auto af = [&](size_t n, float** p) -> int { *p = (float*)c.ar->alloc(n * 4); if (!*p) WDM_FAIL(WDM_ENOMEM, "workspace too small"); return WDM_OK; };
    WDM_TRY(af((size_t)n_t * cfg.ch, &emb));
    WDM_TRY(af((size_t)n_t * L.temb_ch, &t0));
    WDM_TRY(af((size_t)n_t * L.temb_ch, &t1));
    if (!c.dry) {
        WDM_TRY(k_timestep_embedding(t, n_t, cfg.ch, emb, c.s));
        const int temb_ch = L.temb_ch;
        auto pf = [&](int pi) { return (const float*)(packed + slots[pi].off); };
        WDM_TRY(k_linear(emb, n_t, cfg.ch, pf(L.d0w), pf(L.d0b), temb_ch, t0, 2, c.s));
        WDM_TRY(k_linear(t0, n_t, temb_ch, pf(L.d1w), pf(L.d1b), temb_ch, t1, 0, c.s));
        WDM_TRY(k_linear(t1, n_t, temb_ch, (const float*)(packed + temb_w_off), (const float*)(packed + temb_b_off), L.temb_rows, temb_all, 1, c.s));
    }
    c.ar->free(emb); c.ar->free(t0); c.ar->free(t1);
    return WDM_OK;
}

int wdm_unet::forward(Ctx& c, const void* x96, const float* t, int n_t, float* eps_out, const float* temb_pre) {
    const int nres = cfg.n_levels, nrb = cfg.num_res_blocks, R = cfg.resolution;
    const auto &down_res = L.down_res, &up_res = L.up_res;
    const auto &down_attn = L.down_attn, &up_attn = L.up_attn;
    const Res &mid1 = L.mid1, &mid2 = L.mid2;
    const Attn& mid_attn = L.mid_attn;
    const int cin_pad = convd[L.conv_in.idx].cin;      // conv_in's K dimension in the packed matrix
    // every map that carries an AttnBlock, before the first launch (and in the dry run, so the workspace query of such a config fails with the same message)
    for (int l = 0; l < nres; ++l)
        if (!down_attn[l].empty() || !up_attn[l].empty() || l == nres - 1) WDM_TRY(attn_tokens_check(R >> l, R >> l));
    // ---- timestep embedding MLP + every block's temb projection (depends only on t): computed here, or taken from a table the caller made for
    // all the timesteps of a sampling run at once (temb_pre: one row, shared by the images)
    float* temb_all = nullptr;
    if (temb_pre) { temb_all = const_cast<float*>(temb_pre); n_t = 1; }
    else {
        temb_all = (float*)c.ar->alloc((size_t)n_t * L.temb_rows * 4);
        if (!temb_all) WDM_FAIL(WDM_ENOMEM, "workspace too small");
        WDM_TRY(temb_table(c, t, n_t, temb_all));
    }

    Tens x;
    x.p = (void*)x96; x.C = cfg.in_channels; x.H = R; x.W = R; x.xs = cfg.in_channels;
    void* xpad = nullptr;
    if (cin_pad != cfg.in_channels) {      // input width not a multiple of the K slab: zero-padded copy (the weights carry zero columns)
        xpad = c.ar->alloc((size_t)c.B * R * R * cin_pad * dsize(c.dtype));
        if (!xpad) WDM_FAIL(WDM_ENOMEM, "workspace too small (padded input)");
        if (!c.dry) WDM_TRY(k_pad_channels(x96, cfg.in_channels, cin_pad, xpad, (long long)c.B * R * R, c.dtype, c.s));
        x.p = xpad; x.C = cin_pad; x.xs = cin_pad;
    }
    std::vector<Tens> hs;
    Tens h;
    // wdm_unet_forward_taps: a layer's output (and the normalised copy its producer wrote for the consumer, where it wrote one) copied to the caller right behind the
    // launch that produced it, on the same stream -- before the arena can hand the memory to anything else.  Without tap arrays: a counter, nothing launched
    size_t ti = 0;
    auto tap = [&](const Tens& o) -> int {
        const size_t i = ti++;
        if (c.dry || (!c.taps && !c.nrm_taps)) return WDM_OK;
        if (i >= taps.size() || o.C != taps[i].C || o.H != taps[i].H || o.W != taps[i].W || o.xs != o.C) WDM_FAIL(WDM_ESTATE, "internal: tap %zu does not match the tap list", i);
        const size_t bytes = (size_t)c.B * o.H * o.W * o.C * dsize(c.dtype);
        if (c.taps && c.taps[i]) WDM_HIP(hipMemcpyAsync(c.taps[i], o.p, bytes, hipMemcpyDeviceToDevice, c.s));
        if (c.nrm_taps && c.nrm_taps[i] && o.nrm) WDM_HIP(hipMemcpyAsync(c.nrm_taps[i], o.nrm, bytes, hipMemcpyDeviceToDevice, c.s));
        return WDM_OK;
    };
    WDM_TRY(run_conv(c, cw(L.conv_in), MODE_S1, {.x0 = &x, .stats = true}, &h));
    WDM_TRY(tap(h));
    if (xpad) c.ar->free(xpad);
    hs.push_back(h);
    for (int l = 0; l < nres; ++l) {
        for (int b = 0; b < nrb; ++b) {
            Tens o;
            // the consumer of the block's output, when it normalises in a pass of its own (an AttnBlock; the next ResnetBlock on the <= 8 x 8 maps): the block's
            // conv2 writes that norm too where its kernel holds whole images x groups per tile (run_conv: on) -- no gn_finalize_apply launch then
            NormW nn; int nn_silu = 0; bool have_nn = false;
            const int hw_l = (R >> l) * (R >> l);
            if (!down_attn[l].empty()) { nn = aw(down_attn[l][b]).n; have_nn = true; }
            else if (hw_l <= 64) {           // the levels whose ResnetBlocks normalise in a pass (blocks.hip: GN_PASS_MAX_HW)
                if (b + 1 < nrb) { nn = rw(down_res[l][b + 1], temb_all, n_t).n1; nn_silu = 1; have_nn = true; }
                else if (l == nres - 1) { nn = rw(mid1, temb_all, n_t).n1; nn_silu = 1; have_nn = true; }
            }
            WDM_TRY(run_resblock(c, rw(down_res[l][b], temb_all, n_t), hs.back(), nullptr, &o, have_nn ? &nn : nullptr, nn_silu));
            WDM_TRY(tap(o));
            if (!down_attn[l].empty()) {
                Tens o2;
                WDM_TRY(run_attn(c, aw(down_attn[l][b]), o, &o2));
                WDM_TRY(tap(o2));
                free_tens(c, o);
                o = o2;
            }
            hs.push_back(o);
        }
        if (l != nres - 1) {
            Tens o;
            WDM_TRY(run_conv(c, cw(L.down_ds[l]), MODE_S2, {.x0 = &hs.back(), .stats = true}, &o));
            WDM_TRY(tap(o));
            hs.push_back(o);
        }
    }
    // ---- middle (input stays on the skip stack)
    Tens m1, m2;
    const NormW mid_n = aw(mid_attn).n;
    WDM_TRY(run_resblock(c, rw(mid1, temb_all, n_t), hs.back(), nullptr, &m1, &mid_n, 0));
    WDM_TRY(tap(m1));
    WDM_TRY(run_attn(c, aw(mid_attn), m1, &m2));
    WDM_TRY(tap(m2));
    free_tens(c, m1);
    WDM_TRY(run_resblock(c, rw(mid2, temb_all, n_t), m2, nullptr, &h));
    WDM_TRY(tap(h));
    free_tens(c, m2);
    // ---- up path: ResnetBlock on cat([h, skip]) without materialising the concat
    for (int l = nres - 1; l >= 0; --l) {
        for (int b = 0; b <= nrb; ++b) {
            Tens skip = hs.back();
            hs.pop_back();
            Tens o;
            NormW nn;
            if (!up_attn[l].empty()) nn = aw(up_attn[l][b]).n;
            WDM_TRY(run_resblock(c, rw(up_res[l][b], temb_all, n_t), h, &skip, &o, up_attn[l].empty() ? nullptr : &nn, 0));
            WDM_TRY(tap(o));
            free_tens(c, h);
            free_tens(c, skip);
            h = o;
            if (!up_attn[l].empty()) {
                Tens o2;
                WDM_TRY(run_attn(c, aw(up_attn[l][b]), h, &o2));
                WDM_TRY(tap(o2));
                free_tens(c, h);
                h = o2;
            }
        }
        if (l != 0) {
            Tens o;
            WDM_TRY(run_conv(c, cw(L.up_us[l]), MODE_UPS, {.x0 = &h, .stats = true}, &o));
            WDM_TRY(tap(o));
            free_tens(c, h);
            h = o;
        }
    }
    // ---- norm_out -> SiLU -> conv_out, written as NCHW fp32 (the reference's output layout)
    {
        float *sc, *sh;
        WDM_TRY(run_gn(c, nw(L.norm_out), h, nullptr, 1, &sc, &sh));
        Tens dummy;
        WDM_TRY(run_conv(c, cw(L.conv_out), MODE_S1, {.x0 = &h, .scale = sc, .shift = sh, .y_mode = Y_NCHW_F32, .y_ext = eps_out}, &dummy));
        c.ar->free(sc); c.ar->free(sh);
    }
    free_tens(c, h);
    if (!temb_pre) c.ar->free(temb_all);
    if (!hs.empty()) WDM_FAIL(WDM_ESTATE, "internal: skip stack not empty (%zu)", hs.size());
    if (ti != taps.size()) WDM_FAIL(WDM_ESTATE, "internal: %zu layer outputs, the tap list has %zu", ti, taps.size());
    return WDM_OK;
}

// =================================================================================================
// C ABI
// =================================================================================================

extern "C" {

int wdm_abi_version(void) { return WDM_ABI_VERSION; }
const char* wdm_last_error(void) { return wdm::get_error(); }

int wdm_create(int device, wdm_handle** out) {
    if (!out) WDM_FAIL(WDM_EINVAL, "wdm_create: null out");
    int n = 0;
    WDM_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) WDM_FAIL(WDM_EINVAL, "wdm_create: device %d of %d", device, n);
    hipDeviceProp_t prop;
    WDM_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) WDM_FAIL(WDM_EINVAL, "wdm_create: device is %s, this library is built for gfx950 only", prop.gcnArchName);
    *out = new wdm_handle{device};
    return WDM_OK;
}
int wdm_destroy(wdm_handle* h) { delete h; return WDM_OK; }

int wdm_unet_create(wdm_handle* h, const wdm_unet_config* cfg, wdm_unet** out) {
    if (!cfg || !out) WDM_FAIL(WDM_EINVAL, "wdm_unet_create: null argument");   // h may be NULL for host-only layout queries
    if (cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->n_attn_res < 0 || cfg->n_attn_res > 8) WDM_FAIL(WDM_EINVAL, "wdm_unet_create: bad level count");
    if (!dtype_valid(cfg->dtype)) WDM_FAIL(WDM_EINVAL, "wdm_unet_create: bad dtype");
    if (!cfg->resamp_with_conv) WDM_FAIL(WDM_EINVAL, "wdm_unet_create: resamp_with_conv=False is not supported");
    if (cfg->ch % 32 || cfg->in_channels < 1) WDM_FAIL(WDM_EINVAL, "wdm_unet_create: ch must be a multiple of 32");
    if (cfg->resolution % (8 << (cfg->n_levels - 1))) WDM_FAIL(WDM_EINVAL, "wdm_unet_create: resolution %d too small for %d levels (coarsest level must be a multiple of 8)", cfg->resolution, cfg->n_levels);
    if (cfg->out_ch < 1) WDM_FAIL(WDM_EINVAL, "wdm_unet_create: out_ch must be positive");
    wdm_unet* u = new wdm_unet();
    u->h = h;
    u->cfg = *cfg;
    int rc = u->build();
    if (rc != WDM_OK) { delete u; return rc; }
    *out = u;
    return WDM_OK;
}
int wdm_unet_destroy(wdm_unet* u) { delete u; return WDM_OK; }
int wdm_unet_num_params(const wdm_unet* u) { return u ? (int)u->L.params.size() : 0; }
int wdm_unet_param_info(const wdm_unet* u, int i, const char** name, int* ndim, int64_t shape[4]) {
    if (!u || !param_info(u->L.params, i, name, ndim, shape)) WDM_FAIL(WDM_EINVAL, "wdm_unet_param_info: index %d out of range", i);
    return WDM_OK;
}
size_t wdm_unet_packed_bytes(const wdm_unet* u) { return u ? u->packed_bytes : 0; }
int wdm_unet_set_packed(wdm_unet* u, void* packed, size_t bytes) {
    if (!u || !packed) WDM_FAIL(WDM_EINVAL, "wdm_unet_set_packed: null argument");
    if (bytes < u->packed_bytes) WDM_FAIL(WDM_ENOMEM, "wdm_unet_set_packed: %zu bytes given, %zu needed", bytes, u->packed_bytes);
    if (((uintptr_t)packed) & 255) WDM_FAIL(WDM_EINVAL, "wdm_unet_set_packed: buffer must be 256-byte aligned");
    u->packed = (char*)packed;
    for (auto& p : u->slots) p.loaded = false;
    u->all_loaded = false;
    return WDM_OK;
}
int wdm_unet_load_param(wdm_unet* u, const char* name, const float* dev_src, int64_t numel, void* stream) {
    if (!u || !name || !dev_src) WDM_FAIL(WDM_EINVAL, "wdm_unet_load_param: null argument");
    if (!u->packed) WDM_FAIL(WDM_ESTATE, "wdm_unet_load_param: call wdm_unet_set_packed first");
    auto it = u->index.find(name);
    if (it == u->index.end()) WDM_FAIL(WDM_ENOTFOUND, "unknown parameter '%s'", name);
    ParamSlot& p = u->slots[it->second];
    const ParamDesc& desc = u->L.params[it->second];
    if (numel != desc.numel()) WDM_FAIL(WDM_EINVAL, "parameter '%s': %lld elements given, %lld expected", name, (long long)numel, (long long)desc.numel());
    hipStream_t s = (hipStream_t)stream;
    if (p.kind == PK_CONV) {
        const int cout = (int)desc.shape[0], cin = (int)desc.shape[1], k = (int)desc.shape[2];
        // (an Upsample conv is ALSO packed as pre-summed sub-pixel taps, up to four weights each, k_pack_up4: a quarter of the range keeps every sum inside it -- ADVICE r5)
        if (u->cfg.dtype == WDM_F16) WDM_TRY(u->check_f16_range(dev_src, numel, name, s, p.up4_off ? 65504.0f / 4 : 65504.0f));
        WDM_TRY(k_pack_conv(dev_src, cout, cin, k, u->packed + p.off, p.rows_total, p.row_off, p.zero_tail ? 1 : 0, u->cfg.dtype, s, p.cin_dst));
        if (p.sm_off) WDM_TRY(k_pack_conv_sm(dev_src, cout, cin, u->packed + p.sm_off, p.rows_total, s, u->cfg.dtype));
        if (p.up4_off) WDM_TRY(k_pack_up4(dev_src, cout, cin, u->packed + p.up4_off, p.rows_total, s, u->cfg.dtype));
    } else {
        WDM_TRY(k_copy_f32(dev_src, (float*)(u->packed + p.off) + p.row_off, numel, s));
    }
    p.loaded = true;
    if (p.fold >= 0) {
        const int rc = u->refold(p, dev_src, s);
        if (rc != WDM_OK) {                   // the folded operand was not rebuilt: this tensor does not count as loaded, and nothing runs until it is
            p.loaded = false;
            u->all_loaded = false;
            return rc;
        }
    }
    bool all = true;
    for (auto& q : u->slots) all = all && q.loaded;
    u->all_loaded = all;
    return WDM_OK;
}
int wdm_unet_mark_loaded(wdm_unet* u) {
    if (!u || !u->packed) WDM_FAIL(WDM_ESTATE, "wdm_unet_mark_loaded: no packed buffer");
    for (auto& p : u->slots) p.loaded = true;
    u->all_loaded = true;
    return WDM_OK;
}
size_t wdm_unet_workspace_bytes(const wdm_unet* u, int B) {
    if (!u || B <= 0) return 0;
    Arena ar = Arena::dry();
    Ctx c{nullptr, u->cfg.dtype, B, &ar, true};
    int rc = const_cast<wdm_unet*>(u)->forward(c, (const void*)(uintptr_t)4096, nullptr, 1, nullptr);
    // n_t = B needs B-1 more rows of temb scratch than n_t = 1: account for the larger case
    if (rc != WDM_OK) return 0;
    const size_t extra = (size_t)(B - 1) * (u->cfg.ch + 2 * (size_t)u->L.temb_ch + u->L.temb_rows) * 4 + 4096;
    return ar.peak() + align_up(extra, 256);
}
int wdm_unet_temb_rows(const wdm_unet* u) { return u ? u->L.temb_rows : 0; }
int wdm_unet_temb_table(wdm_unet* u, const float* t, int n, float* temb_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!u || !t || !temb_out || !workspace || n <= 0) WDM_FAIL(WDM_EINVAL, "wdm_unet_temb_table: null argument");
    if (!u->all_loaded) WDM_FAIL(WDM_ESTATE, "wdm_unet_temb_table: parameters not loaded");
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_unet_temb_table: workspace must be 256-byte aligned");
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, u->cfg.dtype, 1, &ar, false};
    return u->temb_table(c, t, n, temb_out);
}
int wdm_unet_forward_temb(wdm_unet* u, const void* x96, const float* temb_row, int B, float* eps_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!u || !x96 || !temb_row || !eps_out || !workspace) WDM_FAIL(WDM_EINVAL, "wdm_unet_forward_temb: null argument");
    if (!u->all_loaded) WDM_FAIL(WDM_ESTATE, "wdm_unet_forward_temb: parameters not loaded");
    if (B <= 0) WDM_FAIL(WDM_EINVAL, "wdm_unet_forward_temb: B=%d", B);
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_unet_forward_temb: workspace must be 256-byte aligned");
    // (Round 3 could replay this call as a captured hipGraph -- WDM_GRAPH=1 --: 115.8 / 116.0 img/s against 116.2 / 116.1 eager at the full 100 steps.  The host
    // is never the bound (one C call per UNet forward) and a graph node pays the same kernel-to-kernel gap as an eager launch; removed in round 4.)
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, u->cfg.dtype, B, &ar, false};
    return u->forward(c, x96, nullptr, 1, eps_out, temb_row);
}
int wdm_unet_forward(wdm_unet* u, const void* x96, const float* t, int n_t, int B, float* eps_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!u || !x96 || !t || !eps_out || !workspace) WDM_FAIL(WDM_EINVAL, "wdm_unet_forward: null argument");
    if (!u->all_loaded) WDM_FAIL(WDM_ESTATE, "wdm_unet_forward: parameters not loaded");
    if (B <= 0 || (n_t != 1 && n_t != B)) WDM_FAIL(WDM_EINVAL, "wdm_unet_forward: n_t=%d must be 1 or B=%d", n_t, B);
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_unet_forward: workspace must be 256-byte aligned");
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, u->cfg.dtype, B, &ar, false};
    return u->forward(c, x96, t, n_t, eps_out);
}
int wdm_unet_num_taps(const wdm_unet* u) { return u ? (int)u->taps.size() : 0; }
int wdm_unet_tap_info(const wdm_unet* u, int i, const char** name, int* C, int* H, int* W, int* kind, int* in0, int* in1) {
    if (!u || i < 0 || i >= (int)u->taps.size()) WDM_FAIL(WDM_EINVAL, "wdm_unet_tap_info: index %d out of range", i);
    const TapD& t = u->taps[i];
    if (name) *name = t.name.c_str();
    if (C) *C = t.C;
    if (H) *H = t.H;
    if (W) *W = t.W;
    if (kind) *kind = t.kind;
    if (in0) *in0 = t.in0;
    if (in1) *in1 = t.in1;
    return WDM_OK;
}
int wdm_unet_forward_taps(wdm_unet* u, const void* x96, const float* t, int n_t, int B, float* eps_out, void* const* taps, void* const* nrm_taps, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (!u || !x96 || !t || !eps_out || !workspace) WDM_FAIL(WDM_EINVAL, "wdm_unet_forward_taps: null argument");
    if (!u->all_loaded) WDM_FAIL(WDM_ESTATE, "wdm_unet_forward_taps: parameters not loaded");
    if (B <= 0 || (n_t != 1 && n_t != B)) WDM_FAIL(WDM_EINVAL, "wdm_unet_forward_taps: n_t=%d must be 1 or B=%d", n_t, B);
    if (((uintptr_t)workspace) & 255) WDM_FAIL(WDM_EINVAL, "wdm_unet_forward_taps: workspace must be 256-byte aligned");
    Arena ar(workspace, workspace_bytes);
    Ctx c{(hipStream_t)stream, u->cfg.dtype, B, &ar, false, taps, nrm_taps};
    return u->forward(c, x96, t, n_t, eps_out);
}

}  // extern "C"

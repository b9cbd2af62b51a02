// The layers of the two networks, described once for the sampling and the training engines alike: which parameters exist, under which state_dict names, in
// which order, and which of them each layer owns.  Host-only (no HIP header): an engine lays its own storage out in a table parallel to `params` (same
// index) and reads the topology from the typed records, whose members are indices into `params`.
//   UNetLayout: the reference's DiffusionUNet (models/unet.py:197-307);  HfrmLayout: its HFRM (models/arch.py:132-253)
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wavedm.h"

namespace wdm {

struct ParamDesc {
    std::string name;
    int ndim = 0;
    int64_t shape[4] = {0, 0, 0, 0};
    int64_t numel() const { int64_t n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i]; return n; }
};
inline ParamDesc param_desc(const std::string& name, std::initializer_list<int64_t> shp) {
    ParamDesc p; p.name = name; p.ndim = (int)shp.size(); int i = 0;
    for (auto v : shp) p.shape[i++] = v;
    return p;
}
// the body of every *_param_info: entry i of a parameter list (false: i out of range)
inline bool param_info(const std::vector<ParamDesc>& params, int i, const char** name, int* ndim, int64_t shape[4]) {
    if (i < 0 || i >= (int)params.size()) return false;
    const ParamDesc& p = params[i];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = p.ndim;
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = p.shape[k];
    return true;
}

// ---- DiffusionUNet -------------------------------------------------------------------------------------------------------------------------------------
struct UNetLayout {
    struct Conv { int w = -1, b = -1; int cin = 0, cout = 0, k = 0; int idx = -1; };      // idx: position in `convs`
    struct Norm { int g = -1, b = -1; int c = 0; };
    // temb_row: first row of the block's temb_proj in the concatenated [temb_rows][temb_ch] matrix;  layer: position in construction order (the dropout counter)
    struct Res { int cin = 0, cout = 0; Norm n1, n2; Conv c1, c2, nin; bool has_nin = false; int temb_row = 0, layer = 0; };
    struct Attn { int c = 0; Norm n; Conv q, k, v, proj; };
    struct TembProj { std::string name; int cout; };

    // temb.dense.*, conv_in, the down path, mid, the up path (in execution order), norm_out, conv_out.  The temb_proj Linear layers are NOT in it: the engines keep
    // them as one concatenated matrix and list them last, each in its own order (sampler: weight, bias per layer; trainer: all weights, then all biases)
    std::vector<ParamDesc> params;
    int temb_ch = 0, temb_rows = 0, n_res = 0;
    int d0w = -1, d0b = -1, d1w = -1, d1b = -1;       // temb.dense.0 / .1
    Conv conv_in, conv_out;
    Norm norm_out;
    std::vector<std::vector<Res>> down_res, up_res;      // per level
    std::vector<std::vector<Attn>> down_attn, up_attn;   // per level: empty, or one per ResnetBlock
    std::vector<Conv> down_ds, up_us;                    // per level (unused entries have cout == 0)
    Res mid1, mid2;
    Attn mid_attn;
    std::vector<Conv> convs;                             // every conv, in construction order
    std::vector<TembProj> temb_proj;                     // one per ResnetBlock, in construction order (rows of the concatenated matrix in this order)

    ParamDesc temb_proj_weight(const TembProj& e) const { return param_desc(e.name + ".weight", {e.cout, temb_ch}); }
    ParamDesc temb_proj_bias(const TembProj& e) const { return param_desc(e.name + ".bias", {e.cout}); }

    int add(const std::string& name, std::initializer_list<int64_t> shp) { params.push_back(param_desc(name, shp)); return (int)params.size() - 1; }
    Conv add_conv(const std::string& n, int cin, int cout, int k) {
        Conv c; c.cin = cin; c.cout = cout; c.k = k; c.w = add(n + ".weight", {cout, cin, k, k}); c.b = add(n + ".bias", {cout}); c.idx = (int)convs.size();
        convs.push_back(c);
        return c;
    }
    Norm add_norm(const std::string& n, int c) { Norm d; d.c = c; d.g = add(n + ".weight", {c}); d.b = add(n + ".bias", {c}); return d; }
    Res add_res(const std::string& n, int cin, int cout) {
        Res r; r.cin = cin; r.cout = cout; r.has_nin = cin != cout; r.layer = n_res++;
        r.n1 = add_norm(n + ".norm1", cin);
        r.c1 = add_conv(n + ".conv1", cin, cout, 3);
        r.temb_row = temb_rows; temb_rows += cout; temb_proj.push_back({n + ".temb_proj", cout});
        r.n2 = add_norm(n + ".norm2", cout);
        r.c2 = add_conv(n + ".conv2", cout, cout, 3);
        if (r.has_nin) r.nin = add_conv(n + ".nin_shortcut", cin, cout, 1);
        return r;
    }
    Attn add_attn(const std::string& n, int c) {
        Attn a; a.c = c; a.n = add_norm(n + ".norm", c);
        a.q = add_conv(n + ".q", c, c, 1); a.k = add_conv(n + ".k", c, c, 1); a.v = add_conv(n + ".v", c, c, 1); a.proj = add_conv(n + ".proj_out", c, c, 1);
        return a;
    }
};

inline UNetLayout unet_layout(const wdm_unet_config& cfg) {
    UNetLayout L;
    const int ch = cfg.ch, nres = cfg.n_levels, nrb = cfg.num_res_blocks;
    const auto S = [](int v) { return std::to_string(v); };
    auto is_attn = [&](int res) { for (int i = 0; i < cfg.n_attn_res; ++i) if (cfg.attn_resolutions[i] == res) return true; return false; };
    L.temb_ch = ch * 4;
    L.d0w = L.add("temb.dense.0.weight", {L.temb_ch, ch}); L.d0b = L.add("temb.dense.0.bias", {L.temb_ch});
    L.d1w = L.add("temb.dense.1.weight", {L.temb_ch, L.temb_ch}); L.d1b = L.add("temb.dense.1.bias", {L.temb_ch});
    L.conv_in = L.add_conv("conv_in", cfg.in_channels, ch, 3);
    int res = cfg.resolution, block_in = ch;
    L.down_res.resize(nres); L.down_attn.resize(nres); L.down_ds.resize(nres);
    L.up_res.resize(nres); L.up_attn.resize(nres); L.up_us.resize(nres);
    for (int l = 0; l < nres; ++l) {
        block_in = ch * (l == 0 ? 1 : cfg.ch_mult[l - 1]);
        const int block_out = ch * cfg.ch_mult[l];
        for (int b = 0; b < nrb; ++b) { L.down_res[l].push_back(L.add_res("down." + S(l) + ".block." + S(b), block_in, block_out)); block_in = block_out; }
        if (is_attn(res)) for (int b = 0; b < nrb; ++b) L.down_attn[l].push_back(L.add_attn("down." + S(l) + ".attn." + S(b), block_out));
        if (l != nres - 1) { L.down_ds[l] = L.add_conv("down." + S(l) + ".downsample.conv", block_in, block_in, 3); res /= 2; }
    }
    L.mid1 = L.add_res("mid.block_1", block_in, block_in);
    L.mid_attn = L.add_attn("mid.attn_1", block_in);
    L.mid2 = L.add_res("mid.block_2", block_in, block_in);
    for (int l = nres - 1; l >= 0; --l) {
        const int block_out = ch * cfg.ch_mult[l];
        int skip_in = ch * cfg.ch_mult[l];
        for (int b = 0; b <= nrb; ++b) {
            if (b == nrb) skip_in = ch * (l == 0 ? 1 : cfg.ch_mult[l - 1]);
            L.up_res[l].push_back(L.add_res("up." + S(l) + ".block." + S(b), block_in + skip_in, block_out));
            block_in = block_out;
        }
        if (is_attn(res)) for (int b = 0; b <= nrb; ++b) L.up_attn[l].push_back(L.add_attn("up." + S(l) + ".attn." + S(b), block_out));
        if (l != 0) { L.up_us[l] = L.add_conv("up." + S(l) + ".upsample.conv", block_in, block_in, 3); res *= 2; }
    }
    L.norm_out = L.add_norm("norm_out", block_in);
    L.conv_out = L.add_conv("conv_out", block_in, cfg.out_ch, 3);
    return L;
}

// ---- HFRM ----------------------------------------------------------------------------------------------------------------------------------------------
struct HfrmLayout {
    struct Conv { int w = -1, b = -1; int cin = 0, cout = 0, k = 1; };      // b == -1: no bias
    // w / b: conv1 .. conv5 (conv2 is the depthwise 3x3);  idx: position in registration order over encoders, decoders, mid_blks
    struct Block { int d = 0, idx = 0; int beta, gamma, w[5], b[5], caw, cab, n1w, n1b, n2w, n2b; };

    std::vector<ParamDesc> params;      // the reference's registration order (arch.py:206-233): conv_in, encoders, decoders, mid_blks, ups, downs, conv_out
    Conv conv_in, conv_out;
    std::vector<std::vector<Block>> enc, dec;      // per level
    std::vector<Block> mid;
    std::vector<Conv> ups, downs;                  // ups: 1x1 d -> 2d without bias (+ PixelShuffle);  downs: 2x2 stride-2 d -> 2d
    int n_blocks = 0;

    int add(const std::string& name, std::initializer_list<int64_t> shp) { params.push_back(param_desc(name, shp)); return (int)params.size() - 1; }
    Conv add_conv(const std::string& n, int cin, int cout, int k, bool bias = true) {
        Conv c; c.cin = cin; c.cout = cout; c.k = k; c.w = add(n + ".weight", {cout, cin, k, k});
        if (bias) c.b = add(n + ".bias", {cout});
        return c;
    }
    Block add_block(const std::string& n, int d) {
        Block b; b.d = d; b.idx = n_blocks++;
        b.beta = add(n + ".beta", {1, d, 1, 1}); b.gamma = add(n + ".gamma", {1, d, 1, 1});
        const int co[5] = {2 * d, 2 * d, d, 2 * d, d}, ci[5] = {d, 1, d, d, d}, kk[5] = {1, 3, 1, 1, 1};
        auto conv = [&](int k) { const Conv c = add_conv(n + ".conv" + std::to_string(k + 1), ci[k], co[k], kk[k]); b.w[k] = c.w; b.b[k] = c.b; };
        conv(0); conv(1); conv(2);
        b.caw = add(n + ".channel_attn.chan_conv.weight", {d, d, 1, 1}); b.cab = add(n + ".channel_attn.chan_conv.bias", {d});
        conv(3); conv(4);
        b.n1w = add(n + ".norm1.weight", {d}); b.n1b = add(n + ".norm1.bias", {d});
        b.n2w = add(n + ".norm2.weight", {d}); b.n2b = add(n + ".norm2.bias", {d});
        return b;
    }
    // f(block) for every block in registration order
    template <typename F> void for_each_block(F&& f) const {
        for (auto& lv : enc) for (auto& b : lv) f(b);
        for (auto& lv : dec) for (auto& b : lv) f(b);
        for (auto& b : mid) f(b);
    }
};

inline HfrmLayout hfrm_layout(const wdm_hfrm_config& cfg) {
    HfrmLayout L;
    const int dim = cfg.dim;
    const auto S = [](int v) { return std::to_string(v); };
    L.conv_in = L.add_conv("conv_in", cfg.in_channel, dim, 3);
    int d = dim;
    L.enc.resize(cfg.n_enc); L.dec.resize(cfg.n_dec);
    for (int i = 0; i < cfg.n_enc; ++i) {
        for (int j = 0; j < cfg.enc_blk_nums[i]; ++j) L.enc[i].push_back(L.add_block("encoders." + S(i) + "." + S(j), d));
        d *= 2;
    }
    const int dmid = d;
    for (int i = 0; i < cfg.n_dec; ++i) {
        d /= 2;
        for (int j = 0; j < cfg.dec_blk_nums[i]; ++j) L.dec[i].push_back(L.add_block("decoders." + S(i) + "." + S(j), d));
    }
    for (int j = 0; j < cfg.mid_blk_num; ++j) L.mid.push_back(L.add_block("mid_blks." + S(j), dmid));
    d = dmid;
    for (int i = 0; i < cfg.n_dec; ++i) { L.ups.push_back(L.add_conv("ups." + S(i) + ".0", d, 2 * d, 1, false)); d /= 2; }
    d = dim;
    for (int i = 0; i < cfg.n_enc; ++i) { L.downs.push_back(L.add_conv("downs." + S(i), d, 2 * d, 2)); d *= 2; }
    L.conv_out = L.add_conv("conv_out", dim, cfg.in_channel, 3);
    return L;
}

}  // namespace wdm

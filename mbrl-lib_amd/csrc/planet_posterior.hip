// planet_posterior.hip -- the PlaNet posterior update on the device (hipets_planet_posterior_set_model / hipets_planet_encode /
// hipets_planet_posterior_update): the host side of planet_posterior.hpp's kernels.  The layer table and the dealing rule, the packing,
// the chain of product launches, the entry points.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "engine.hpp"
#include "planet_posterior.hpp"

namespace hipets {

namespace {

// The dealing rule.  At ONE image a layer has ceil(P / 16) row tiles and ceil(column tiles / 4) column slices; where that is fewer than
// kTargetWorkgroups workgroups -- the deep layers: few rows, much weight, and one CU's L1 fill rate is what bounds a one-tile kernel
//  -- K is cut into equal ranges of whole k-blocks, no shorter than kMinRangeBlocks (a range's gather and epilogue
// must stay small next to its products).  Only the layer's shape enters: the ranges, and with them the summation order of every output
// element, are the same for every n_env and every slot of the batch.
constexpr int kTargetWorkgroups = 64;
constexpr int kMinRangeBlocks = 8;

void deal_layer(PosteriorLayer& l) {
    const int P = l.OH * l.OW, row_tiles = (P + kTile - 1) / kTile;
    const int slices = (l.Np / kTile + kProdWaves - 1) / kProdWaves;
    const int nkb = l.Kp / kKChunk;
    const int want = (kTargetWorkgroups + row_tiles * slices - 1) / (row_tiles * slices);
    const int most = std::max(1, nkb / kMinRangeBlocks);
    const int S = std::min(want, most);
    l.kb_per_split = (nkb + S - 1) / S;
    l.splits = (nkb + l.kb_per_split - 1) / l.kb_per_split;  // (every range holds at least one k-block)
}

// floats of a layer's output for n_env images, partial sums included
size_t layer_floats(const PosteriorLayer& l, int n_env) { return (size_t)l.splits * n_env * l.OH * l.OW * l.C_out; }

// layer i's output as its consumer indexes it: the next conv layer by (position, channel), everything behind the last conv layer by the
// flattened index alone
ProdSrc layer_as_source(const PosteriorSnapshot& ps, int i, const float* act, const float* bias, int n_env) {
    const PosteriorLayer& l = ps.layers[i];
    const int P = l.OH * l.OW;
    ProdSrc s{};
    s.p = act; s.bias = bias + l.b_off; s.kind = SRC_ACT; s.S = l.splits; s.relu = l.relu;
    s.img_stride = (long long)P * l.C_out; s.split_stride = (long long)n_env * P * l.C_out;
    if (l.chw_out) { s.pos_stride = 0; s.c_stride = 1; s.bias_div = P; }  // (the consumer's "channel" is the flattened (c, oh, ow) index)
    else { s.pos_stride = l.C_out; s.c_stride = 1; s.bias_div = 1; }
    return s;
}

// layers [0, upto) of the chain on `obs`; returns the buffer that holds the last one's output in *last
int run_chain(hipets_engine* e, const void* obs, int obs_is_u8, int n_env, int upto, const float** last, hipStream_t st) {
    PosteriorSnapshot& ps = e->posterior;
    size_t need = 0;
    for (int i = 0; i < ps.n_layers; ++i) need = std::max(need, layer_floats(ps.layers[i], n_env));
    if (ps.act[0].ensure(need * 4) || ps.act[1].ensure(need * 4)) return 1;
    const float* bias = ps.b.as<float>();
    for (int i = 0; i < upto; ++i) {
        const PosteriorLayer& l = ps.layers[i];
        ProdArgs a{};
        if (i == 0) {
            a.src.p = obs; a.src.kind = obs_is_u8 ? SRC_U8_IMAGE : SRC_F32_IMAGE; a.src.S = 1; a.src.bias_div = 1;
            a.src.img_stride = (long long)ps.C * ps.H * ps.W; a.src.pos_stride = 1; a.src.c_stride = ps.H * ps.W;
        } else {
            a.src = layer_as_source(ps, i - 1, ps.act[(i - 1) & 1].as<float>(), bias, n_env);
        }
        const int P = l.OH * l.OW;
        a.w = ps.w.as<float>() + l.w_off; a.bias = bias + l.b_off; a.out = ps.act[i & 1].as<float>();
        a.M = (long long)n_env * P;
        a.o_img = (long long)P * l.C_out; a.split_stride = (long long)n_env * P * l.C_out;
        if (l.chw_out) { a.o_pos = 1; a.o_c = P; } else { a.o_pos = l.C_out; a.o_c = 1; }
        a.C_in = l.C_in; a.C_out = l.C_out; a.ksz = l.k; a.stride = l.stride; a.W = l.W; a.OW = l.OW; a.P = P;
        a.K = l.K; a.Kp = l.Kp; a.Np = l.Np; a.S = l.splits; a.kb_per_split = l.kb_per_split; a.relu = l.relu;
        const dim3 grid((unsigned)((a.M + kTile - 1) / kTile), (unsigned)((l.Np / kTile + kProdWaves - 1) / kProdWaves), (unsigned)l.splits);
        hipLaunchKernelGGL(posterior_product_kernel, grid, dim3(kProdThreads), 0, st, a);
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "posterior product kernel launch failed: %s", hipGetErrorString(err));
    *last = ps.act[(upto - 1) & 1].as<float>();
    return 0;
}

int check_call(const hipets_engine* e, const void* obs, int n_env) {
    if (!e || !e->posterior.set) return fail("engine has no PlaNet posterior model (call hipets_planet_posterior_set_model)");
    if (!obs) return fail("null argument");
    if (n_env < 1 || n_env > HIPETS_ENCODER_MAX_ENV) return fail("n_env %d outside [1, %d]", n_env, HIPETS_ENCODER_MAX_ENV);
    return 0;
}

bool outside(int v, int lo, int hi) { return v < lo || v > hi; }

}  // namespace

}  // namespace hipets

using namespace hipets;

extern "C" {

int hipets_planet_posterior_set_model(hipets_engine* e, int32_t n_conv, const int32_t* conv_dims, const int32_t* image_chw, int32_t enc_size,
                                      int32_t latent, int32_t action, int32_t belief, int32_t hidden, float min_std, const void* ptrs,
                                      int32_t n_ptrs) {
    if (!e) return fail("null engine");
    PosteriorSnapshot& ps = e->posterior;
    ps.set = false;  // (a refused set leaves no posterior model behind)
    if (!conv_dims || !image_chw || !ptrs) return fail("null argument");
    if (outside(n_conv, 1, HIPETS_ENCODER_MAX_CONVS)) return fail("encoder has %d conv layers, outside [1, %d]", n_conv, HIPETS_ENCODER_MAX_CONVS);
    if (n_ptrs != 2 * n_conv + 12) return fail("posterior pointer table holds %d entries, expected %d", n_ptrs, 2 * n_conv + 12);
    if (outside(image_chw[0], 1, HIPETS_ENCODER_MAX_CHANNELS) || outside(image_chw[1], 1, HIPETS_ENCODER_MAX_IMAGE) || outside(image_chw[2], 1, HIPETS_ENCODER_MAX_IMAGE))
        return fail("image [%d, %d, %d] outside [%d, %d, %d]", image_chw[0], image_chw[1], image_chw[2], HIPETS_ENCODER_MAX_CHANNELS, HIPETS_ENCODER_MAX_IMAGE, HIPETS_ENCODER_MAX_IMAGE);
    if (outside(enc_size, 1, HIPETS_ENCODER_MAX_FLAT)) return fail("encoding size %d outside [1, %d]", enc_size, HIPETS_ENCODER_MAX_FLAT);
    if (outside(latent, 1, HIPETS_POSTERIOR_MAX_LATENT) || outside(action, 1, HIPETS_POSTERIOR_MAX_ACTION) || outside(belief, 1, HIPETS_POSTERIOR_MAX_BELIEF) ||
        outside(hidden, 1, HIPETS_POSTERIOR_MAX_HIDDEN))
        return fail("posterior sizes (latent %d, action %d, belief %d, hidden %d) outside (%d, %d, %d, %d)", latent, action, belief, hidden,
                    HIPETS_POSTERIOR_MAX_LATENT, HIPETS_POSTERIOR_MAX_ACTION, HIPETS_POSTERIOR_MAX_BELIEF, HIPETS_POSTERIOR_MAX_HIDDEN);
    if (!(min_std >= 0.f)) return fail("bad min_std");
    const float* const* p = static_cast<const float* const*>(ptrs);
    const float* const* fc = p + 2 * n_conv;
    const float* const* hd = fc + 2;  // w_embed, b_embed, w_ih, b_ih, w_hh, b_hh, w_post1, b_post1, w_post2, b_post2
    for (int i = 0; i < n_ptrs; ++i)
        if (!p[i] && (i < 2 * n_conv || i >= 2 * n_conv + 2)) return fail("posterior pointer %d is null", i);
    if ((fc[0] == nullptr) != (fc[1] == nullptr)) return fail("the encoder's Linear needs weight and bias, or neither");

    // ---- the layer table ----
    ps.n_conv = n_conv; ps.has_fc = fc[0] != nullptr;
    ps.n_layers = n_conv + ps.has_fc + 1;
    ps.C = image_chw[0]; ps.H = image_chw[1]; ps.W = image_chw[2];
    ps.enc = enc_size; ps.latent = latent; ps.action = action; ps.belief = belief; ps.hidden = hidden; ps.min_std = min_std;
    int C = ps.C, H = ps.H, W = ps.W;
    size_t nw = 0, nb = 0;
    auto place = [&](PosteriorLayer& l) {
        l.K = l.C_in * l.k * l.k; l.Kp = pad16(l.K); l.Np = pad16(l.C_out);
        l.w_off = nw; l.b_off = nb;
        nw += (size_t)l.Kp * l.Np; nb += (size_t)l.Np;
        deal_layer(l);
    };
    for (int i = 0; i < n_conv; ++i) {
        const int32_t* d = conv_dims + 4 * i;
        PosteriorLayer& l = ps.layers[i];
        l = PosteriorLayer{};
        l.C_in = d[0]; l.C_out = d[1]; l.k = d[2]; l.stride = d[3]; l.H = H; l.W = W;
        if (l.C_in != C) return fail("conv layer %d reads %d channels, its input has %d", i, l.C_in, C);
        if (outside(l.C_out, 1, HIPETS_ENCODER_MAX_CHANNELS) || outside(l.k, 1, HIPETS_ENCODER_MAX_KERNEL) || outside(l.stride, 1, HIPETS_ENCODER_MAX_STRIDE))
            return fail("conv layer %d (C_out %d, kernel %d, stride %d) outside (%d, %d, %d)", i, l.C_out, l.k, l.stride, HIPETS_ENCODER_MAX_CHANNELS,
                        HIPETS_ENCODER_MAX_KERNEL, HIPETS_ENCODER_MAX_STRIDE);
        if (l.k > H || l.k > W) return fail("conv layer %d: kernel %d does not fit its %d x %d input", i, l.k, H, W);
        l.OH = (H - l.k) / l.stride + 1; l.OW = (W - l.k) / l.stride + 1;
        if ((long long)l.OH * l.OW * l.C_out > HIPETS_ENCODER_MAX_LAYER_FLOATS)
            return fail("conv layer %d has %lld outputs per image, more than %d", i, (long long)l.OH * l.OW * l.C_out, HIPETS_ENCODER_MAX_LAYER_FLOATS);
        l.relu = 1; l.chw_out = i == n_conv - 1;
        place(l);
        C = l.C_out; H = l.OH; W = l.OW;
    }
    ps.flat = C * H * W;
    if (ps.flat > HIPETS_ENCODER_MAX_FLAT) return fail("flattened encoding %d exceeds %d", ps.flat, HIPETS_ENCODER_MAX_FLAT);
    if (!ps.has_fc && ps.flat != enc_size) return fail("no Linear, and the flattened conv output %d is not the encoding size %d", ps.flat, enc_size);
    auto linear = [&](int i, int K, int N) {
        PosteriorLayer& l = ps.layers[i];
        l = PosteriorLayer{};
        l.C_in = K; l.C_out = N;
        place(l);
    };
    if (ps.has_fc) linear(n_conv, ps.flat, enc_size);
    linear(ps.n_layers - 1, enc_size, hidden);  // posterior[0], columns [belief, belief + enc) of its weight, and its bias

    // ---- the head ----
    const int xp = pad16(latent + action), hbp = pad16(belief), g3p = pad16(3 * belief), fp = pad16(hidden), l2p = pad16(2 * latent);
    ps.head_lds = (size_t)kTile * 4 * ((size_t)std::max(xp, fp) + std::max(hbp, l2p) + hbp + 2 * (size_t)g3p + 20);
    if (ps.head_lds > e->lds_max) return fail("posterior head needs %zu bytes of LDS, the limit is %zu", ps.head_lds, e->lds_max);
    const int hk[5] = {latent + action, belief, belief, belief, hidden}, hn[5] = {belief, 3 * belief, 3 * belief, hidden, 2 * latent};
    const int hnp[5] = {hbp, g3p, g3p, fp, l2p};
    const size_t chain_w = nw, chain_b = nb;
    for (int i = 0; i < 5; ++i) {
        ps.head_w[i] = nw - chain_w; ps.head_b[i] = nb - chain_b;
        nw += (size_t)pad16(hk[i]) * hnp[i]; nb += (size_t)hnp[i];
    }

    // ---- pack ----
    hipStream_t st = nullptr;  // (a blocking call on the device's default stream: include/hipets.h, Conventions)
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    if (ps.w.ensure(nw * 4) || ps.b.ensure(nb * 4)) return 1;
    float* wd = ps.w.as<float>();
    float* bd = ps.b.as<float>();
    HCHECK(hipMemsetAsync(wd, 0, nw * 4, st));
    HCHECK(hipMemsetAsync(bd, 0, nb * 4, st));
    auto pack = [&](float* dst, const float* src, int N, int C_in, int ksz, long long src_ld, int np) {
        const long long n = (long long)N * C_in * ksz * ksz;
        hipLaunchKernelGGL(posterior_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, N, C_in, ksz, src_ld, np);
    };
    for (int i = 0; i < ps.n_layers; ++i) {
        const PosteriorLayer& l = ps.layers[i];
        const float *w, *b;
        long long ld = l.K;
        if (i < n_conv) { w = p[2 * i]; b = p[2 * i + 1]; }
        else if (i < ps.n_layers - 1) { w = fc[0]; b = fc[1]; }
        else { w = hd[6] + belief; b = hd[7]; ld = belief + enc_size; }
        pack(wd + l.w_off, w, l.C_out, l.C_in, l.k, ld, l.Np);
        HCHECK(hipMemcpyAsync(bd + l.b_off, b, (size_t)l.C_out * 4, hipMemcpyDeviceToDevice, st));
    }
    const float* hw[5] = {hd[0], hd[2], hd[4], hd[6], hd[8]};
    const float* hb[5] = {hd[1], hd[3], hd[5], nullptr, hd[9]};  // (posterior[0]'s bias travels with its encoding half)
    const long long hld[5] = {latent + action, belief, belief, belief + enc_size, hidden};
    for (int i = 0; i < 5; ++i) {
        pack(wd + chain_w + ps.head_w[i], hw[i], hn[i], hk[i], 1, hld[i], hnp[i]);
        if (hb[i]) HCHECK(hipMemcpyAsync(bd + chain_b + ps.head_b[i], hb[i], (size_t)hn[i] * 4, hipMemcpyDeviceToDevice, st));
    }
    HCHECK(hipGetLastError());
    for (int i = 0; i < 5; ++i) { ps.head_w[i] += chain_w; ps.head_b[i] += chain_b; }
    HCHECK(hipStreamSynchronize(st));  // (the caller's tensors may go away on return, like hipets_planet_set_model's)
    ps.set = true;
    return 0;
}

int hipets_planet_encode(hipets_engine* e, const void* obs, int32_t obs_is_u8, int32_t n_env, float* out_enc) {
    if (check_call(e, obs, n_env)) return 1;
    if (!out_enc) return fail("null argument");
    hipStream_t st = nullptr;  // (a blocking call on the device's default stream: include/hipets.h, Conventions)
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    PosteriorSnapshot& ps = e->posterior;
    const int upto = ps.n_layers - 1;  // (without the posterior's encoding half)
    const float* last = nullptr;
    if (run_chain(e, obs, obs_is_u8, n_env, upto, &last, st)) return 1;
    const ProdSrc s = layer_as_source(ps, upto - 1, last, ps.b.as<float>(), n_env);  // (one position per image: read at position 0)
    const long long n = (long long)n_env * ps.enc;
    hipLaunchKernelGGL(posterior_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s, out_enc, n_env, ps.enc);
    HCHECK(hipGetLastError());
    HCHECK(hipStreamSynchronize(st));  // (the results are complete on return: include/hipets.h, Conventions)
    return 0;
}

int hipets_planet_posterior_update(hipets_engine* e, const void* obs, int32_t obs_is_u8, int32_t n_env, const float* action,
                                   float* latent_inout, float* belief_inout, const float* eps_or_null, const uint8_t* first_mask_or_null) {
    if (check_call(e, obs, n_env)) return 1;
    if (!latent_inout || !belief_inout) return fail("null argument");
    hipStream_t st = nullptr;  // (a blocking call on the device's default stream: include/hipets.h, Conventions)
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    PosteriorSnapshot& ps = e->posterior;
    const float* last = nullptr;
    if (run_chain(e, obs, obs_is_u8, n_env, ps.n_layers, &last, st)) return 1;
    HeadArgs a{};
    a.w = ps.w.as<float>(); a.b = ps.b.as<float>();
    for (int i = 0; i < 5; ++i) { a.w_off[i] = ps.head_w[i]; a.b_off[i] = ps.head_b[i]; }
    a.p1enc = layer_as_source(ps, ps.n_layers - 1, last, a.b, n_env);
    a.action = action; a.eps = eps_or_null; a.first = first_mask_or_null; a.latent = latent_inout; a.belief = belief_inout;
    a.n_env = n_env; a.L = ps.latent; a.A = ps.action; a.Hb = ps.belief; a.F = ps.hidden;
    a.xp = pad16(a.L + a.A); a.hbp = pad16(a.Hb); a.g3p = pad16(3 * a.Hb); a.fp = pad16(a.F); a.l2p = pad16(2 * a.L);
    a.ldX = std::max(a.xp, a.fp) + 4; a.ldE = std::max(a.hbp, a.l2p) + 4; a.ldH = a.hbp + 4; a.ldG = a.g3p + 4;
    a.min_std = ps.min_std;
    if (ps.head_lds > 64 * 1024) {
        static LdsOptIn opted;
        const hipError_t err = full_lds_once(opted, reinterpret_cast<const void*>(posterior_head_kernel), (int)e->lds_max);
        if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "posterior head LDS opt-in failed: %s", hipGetErrorString(err));
    }
    hipLaunchKernelGGL(posterior_head_kernel, dim3((unsigned)((n_env + kTile - 1) / kTile)), dim3(kPolicyThreads), ps.head_lds, st, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "posterior head kernel launch failed: %s", hipGetErrorString(err));
    HCHECK(hipStreamSynchronize(st));  // (the results are complete on return: include/hipets.h, Conventions)
    return 0;
}

}  // extern "C"

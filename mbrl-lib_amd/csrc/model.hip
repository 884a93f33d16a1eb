// model.hip -- model upload of the C ABI (include/hipets.h): hipets_set_model packs the ensemble for the rollout kernels, hipets_planet_set_model
// the PlaNet latent model.  Host code only: the packing kernels are launched through rollout.hip (engine.hpp pack_*).
#include <algorithm>

#include "engine.hpp"
#include "rollout_smem.hpp"

using namespace hipets;

namespace {

// The parametric closed forms of the descriptor (include/hipets.h HIPETS_REW_TERMS / HIPETS_TERM_BOX), checked entry by entry and laid
// out as the kernels read them (all zero: the model has neither).
int read_form_tables(const hipets_model_desc* d, FormTables* ft) {
    const bool terms = d->reward_fn == HIPETS_REW_TERMS, box = d->termination_fn == HIPETS_TERM_BOX;
    if (d->reward_fn < HIPETS_REW_LEARNED || d->reward_fn > HIPETS_REW_TERMS) return fail("unknown reward_fn %d", d->reward_fn);
    if (d->termination_fn < HIPETS_TERM_NONE || d->termination_fn > HIPETS_TERM_BOX) return fail("unknown termination_fn %d", d->termination_fn);
    if (!terms && (d->reward_terms || d->n_reward_terms || d->reward_bias != 0.0f || d->alive_bonus != 0.0f))
        return fail("reward_terms / n_reward_terms / reward_bias / alive_bonus are set but reward_fn %d is not HIPETS_REW_TERMS", d->reward_fn);
    if (!box && (d->term_intervals || d->n_term_intervals || d->term_require_finite))
        return fail("term_intervals / n_term_intervals / term_require_finite are set but termination_fn %d is not HIPETS_TERM_BOX", d->termination_fn);
    if (terms) {
        if (d->n_reward_terms < 0 || d->n_reward_terms > HIPETS_MAX_REWARD_TERMS)
            return fail("n_reward_terms %d outside [0, %d]", d->n_reward_terms, HIPETS_MAX_REWARD_TERMS);
        if (d->n_reward_terms > 0 && !d->reward_terms) return fail("reward_fn TERMS: reward_terms is null for n_reward_terms %d", d->n_reward_terms);
        if (d->alive_bonus != 0.0f && d->termination_fn == HIPETS_TERM_NONE) return fail("alive_bonus %g needs a termination_fn other than NONE", (double)d->alive_bonus);
        int open[HIPETS_TERM_MAX_LEVEL + 1] = {0, 0, 0}, last[HIPETS_TERM_MAX_LEVEL + 1] = {0, 0, 0};  // entries of the open group of a level since it was consumed, its latest entry
        for (int k = 0; k < d->n_reward_terms; ++k) {
            const hipets_reward_term& t = d->reward_terms[k];
            const int fn = HIPETS_TERM_WORD_FN(t.fn), op = HIPETS_TERM_WORD_OP(t.fn), level = HIPETS_TERM_WORD_LEVEL(t.fn);
            if (fn > HIPETS_TERM_FN_SQRT) return fail("reward term %d: unknown fn %d", k, fn);
            if (op > HIPETS_TERM_OP_DIV) return fail("reward term %d: unknown op %d", k, op);
            if (level > HIPETS_TERM_MAX_LEVEL) return fail("reward term %d: level %d outside [0, %d]", k, level, HIPETS_TERM_MAX_LEVEL);
            if (t.source < HIPETS_TERM_SRC_OBS || t.source > HIPETS_TERM_SRC_CONST) return fail("reward term %d: unknown source %d", k, t.source);
            ft->terms[k] = t;
            if (t.source == HIPETS_TERM_SRC_GROUP || t.source == HIPETS_TERM_SRC_CONST) {
                if (t.j >= 0) return fail("reward term %d: j = %d is set on a GROUP / CONST entry", k, t.j);
                if (t.source == HIPETS_TERM_SRC_GROUP) {
                    if (level == HIPETS_TERM_MAX_LEVEL) return fail("reward term %d: GROUP at level %d has no deeper group to consume", k, level);
                    if (!open[level + 1]) return fail("reward term %d: GROUP consumes an empty group (level %d has no entry since it was last consumed)", k, level + 1);
                    open[level + 1] = 0;
                }
                ft->terms[k].i = 0;  // (not read)
            } else {
                const int width = t.source == HIPETS_TERM_SRC_ACT ? d->act_dim : d->obs_dim;
                if (t.i < 0 || t.i >= width) return fail("reward term %d: dim i = %d outside [0, %d)", k, t.i, width);
                if (t.j >= width) return fail("reward term %d: dim j = %d outside [0, %d)", k, t.j, width);
            }
            if (t.j < 0) ft->terms[k].j = -1;
            if (op != HIPETS_TERM_OP_ADD && level > 0 && !open[level]) return fail("reward term %d: mul / div into an empty group (level %d starts at 0)", k, level);
            ++open[level];
            last[level] = k;
            if (t.fn > HIPETS_TERM_FN_ABS || t.source > HIPETS_TERM_SRC_ACT) ft->grouped = 1;  // (t.fn: the whole word)
        }
        for (int level = 1; level <= HIPETS_TERM_MAX_LEVEL; ++level)
            if (open[level]) return fail("reward term %d: the group at level %d is left open at the end of the table", last[level], level);
        ft->n_terms = d->n_reward_terms;
        ft->bias = d->reward_bias;
        ft->alive_bonus = d->alive_bonus;
    }
    if (box) {
        if (d->n_term_intervals < 0 || d->n_term_intervals > HIPETS_MAX_TERM_INTERVALS)
            return fail("n_term_intervals %d outside [0, %d]", d->n_term_intervals, HIPETS_MAX_TERM_INTERVALS);
        if (d->n_term_intervals > 0 && !d->term_intervals) return fail("termination_fn BOX: term_intervals is null for n_term_intervals %d", d->n_term_intervals);
        for (int k = 0; k < d->n_term_intervals; ++k) {
            const hipets_term_interval& iv = d->term_intervals[k];
            if (iv.dim < 0 || iv.dim >= d->obs_dim) return fail("term interval %d: dim %d outside [0, %d)", k, iv.dim, d->obs_dim);
            if (iv.flags & ~(HIPETS_BOX_LO_OPEN | HIPETS_BOX_HI_OPEN)) return fail("term interval %d: unknown flags 0x%x", k, (unsigned)iv.flags);
            if (!(iv.lo <= iv.hi)) return fail("term interval %d: lo %g is not <= hi %g", k, (double)iv.lo, (double)iv.hi);
            ft->intervals[k] = iv;
        }
        ft->n_intervals = d->n_term_intervals;
        ft->require_finite = d->term_require_finite ? 1 : 0;
    }
    return 0;
}

// The column table of a HIPETS_OBS_COLUMNS model (include/hipets.h hipets_set_model_columns), checked entry by entry.
int read_obs_columns(const hipets_model_desc* d, const hipets_obs_column* cols, const int n_cols) {
    if (!cols) return fail("obs_process COLUMNS: cols is null");
    if (n_cols < 1 || n_cols > HIPETS_MAX_OBS_COLUMNS) return fail("n_cols %d outside [1, %d]", n_cols, HIPETS_MAX_OBS_COLUMNS);
    for (int k = 0; k < n_cols; ++k) {
        if (cols[k].dim < 0 || cols[k].dim >= d->obs_dim) return fail("obs column %d: dim %d outside [0, %d)", k, cols[k].dim, d->obs_dim);
        if (cols[k].fn != HIPETS_COL_ID && cols[k].fn != HIPETS_COL_SIN && cols[k].fn != HIPETS_COL_COS) return fail("obs column %d: unknown fn %d", k, cols[k].fn);
    }
    return 0;
}

// hipets_set_model and hipets_set_model_columns: one body.  cols = the column table of a HIPETS_OBS_COLUMNS model, null for every other
// obs_process (the entry points have checked which of the two the descriptor asks for).
int set_model(hipets_engine* e, const hipets_model_desc* d, const hipets_obs_column* cols, const int n_cols, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    if (d->n_layers < 2 || d->n_layers > HIPETS_MAX_LAYERS) return fail("n_layers %d outside [2, %d]", d->n_layers, HIPETS_MAX_LAYERS);
    if (d->n_members < 1 || d->n_members > d->ensemble_size) return fail("n_members %d invalid for ensemble_size %d", d->n_members, d->ensemble_size);
    if (d->obs_dim < 1 || d->act_dim < 1 || d->in_dim < d->act_dim + 1 || d->hid < 1) return fail("bad dimensions");
    if (d->out_dim != d->obs_dim + (d->learned_rewards ? 1 : 0)) return fail("out_dim %d != obs_dim %d + learned_rewards %d", d->out_dim, d->obs_dim, d->learned_rewards);
    const int obs_in = d->in_dim - d->act_dim;
    if (d->obs_process < HIPETS_OBS_NONE || d->obs_process > HIPETS_OBS_COLUMNS) return fail("unknown obs_process %d", d->obs_process);
    if (cols && obs_in != n_cols) return fail("in_dim %d != n_cols %d + act_dim %d", d->in_dim, n_cols, d->act_dim);
    const int expect_in = cols ? n_cols : (d->obs_process == HIPETS_OBS_CARTPOLE_PETS ? d->obs_dim + 1 : d->obs_dim);
    if (obs_in != expect_in) return fail("in_dim %d inconsistent with obs_dim %d / obs_process %d / act_dim %d", d->in_dim, d->obs_dim, d->obs_process, d->act_dim);
    if (d->reward_fn == HIPETS_REW_LEARNED && !d->learned_rewards) return fail("reward_fn LEARNED needs learned_rewards");
    if (d->reward_fn == HIPETS_REW_HALFCHEETAH && d->obs_dim < 3) return fail("halfcheetah reward needs obs_dim >= 3");
    if (d->reward_fn == HIPETS_REW_PUSHER && d->obs_dim < 20) return fail("pusher reward needs obs_dim >= 20");
    if ((d->reward_fn == HIPETS_REW_CARTPOLE || d->termination_fn == HIPETS_TERM_CARTPOLE) && d->obs_dim < 3) return fail("cartpole fns need obs_dim >= 3");
    if ((d->obs_process == HIPETS_OBS_HALFCHEETAH) && d->obs_dim < 3) return fail("halfcheetah obs_process needs obs_dim >= 3");
    if (d->obs_dim < 2 && (d->termination_fn != HIPETS_TERM_NONE || d->reward_fn == HIPETS_REW_CARTPOLE_PETS)) return fail("termination/reward fn needs obs_dim >= 2");
    if (!d->deterministic && (!d->min_logvar || !d->max_logvar)) return fail("logvar bounds missing");
    if (d->ensemble_kind != HIPETS_ENSEMBLE_GAUSSIAN_MLP && d->ensemble_kind != HIPETS_ENSEMBLE_BASIC)
        return fail("unknown ensemble_kind %d", d->ensemble_kind);
    if (d->ensemble_kind == HIPETS_ENSEMBLE_BASIC && d->n_members != d->ensemble_size)
        return fail("BasicEnsemble has no elite subset (basic_ensemble.py:262-266): n_members %d != ensemble_size %d", d->n_members,
                    d->ensemble_size);
    if (d->normalizer != HIPETS_NORM_NONE && (!d->norm_mean || !d->norm_std)) return fail("normalizer stats missing");
    for (int i = 0; i < d->n_members; ++i)
        if (d->members[i] < 0 || d->members[i] >= d->ensemble_size) return fail("member index %d out of range", d->members[i]);
    FormTables forms{};
    if (read_form_tables(d, &forms)) return 1;

    ModelDev md{};
    md.obs_dim = d->obs_dim; md.act_dim = d->act_dim; md.in_dim = d->in_dim; md.out_dim = d->out_dim;
    md.out_total = d->deterministic ? d->out_dim : 2 * d->out_dim;
    md.hid = d->hid; md.n_layers = d->n_layers; md.M = d->n_members; md.obs_in = obs_in;
    md.activation = d->activation; md.slope = d->leaky_slope; md.propagation = d->propagation;
    md.deterministic = d->deterministic; md.obs_process = d->obs_process; md.reward_fn = d->reward_fn;
    md.term_fn = d->termination_fn; md.target_is_delta = d->target_is_delta; md.learned_rewards = d->learned_rewards;
    md.normalizer = d->normalizer;
    md.iid_members = d->ensemble_kind == HIPETS_ENSEMBLE_BASIC ? 1 : 0;
    md.lv_rows = (md.iid_members && !d->deterministic) ? d->n_members : 1;
    auto up16 = [](int x) { return (x + 15) / 16 * 16; };
    long long woff = 0;
    int boff = 0, maxK = 0;
    std::vector<int> Ks(d->n_layers), Ns(d->n_layers);
    std::vector<LayerMeta> lms(d->n_layers);
    for (int l = 0; l < d->n_layers; ++l) {
        Ks[l] = l == 0 ? d->in_dim : d->hid;
        Ns[l] = l == d->n_layers - 1 ? md.out_total : d->hid;
        lms[l].Kp = up16(Ks[l]);
        lms[l].Np = up16(Ns[l]);
        lms[l].woff = woff;
        lms[l].boff = boff;
        lms[l].tail_steps = (Ks[l] - (lms[l].Kp - 16) + 3) / 4;
        lms[l].woff_pairs = -1;
        lms[l].boff_pairs = 0;
        lms[l].pad2_ = 0;
        woff += (long long)lms[l].Kp * lms[l].Np;
        boff += lms[l].Np;
        maxK = std::max(maxK, std::max(lms[l].Kp, lms[l].Np));
    }
    if (!d->deterministic) {  // second pack of the mean / logvar head in "head pair" column order (rollout_types.hpp head_pair_col, KSpec::FUSE)
        LayerMeta& out = lms[d->n_layers - 1];
        out.woff_pairs = woff;
        out.boff_pairs = boff;
        woff += (long long)out.Kp * out.Np;  // ceil(out_dim / 8) column tiles == Np / 16: the pair order never needs more tiles
        boff += out.Np;
    }
    md.precision = d->precision;
    if (d->precision != HIPETS_PREC_F32 && d->precision != HIPETS_PREC_BF16X3 && d->precision != HIPETS_PREC_BF16) return fail("unknown precision %d", d->precision);
    const int pieces = d->precision == HIPETS_PREC_BF16 ? 1 : 3;  // bf16 planes per weight (bf16: piece 0 of the split alone)
    long long w3off = 0;  // 16-byte units
    int max_kc32 = 1;
    for (int l = 0; l < d->n_layers; ++l) {
        lms[l].Kp32 = (Ks[l] + 31) / 32 * 32;
        lms[l].pad_ = 0;
        lms[l].woff3 = w3off;
        w3off += (long long)(lms[l].Np / 16) * (lms[l].Kp32 / 32) * pieces * 64;
        max_kc32 = std::max(max_kc32, lms[l].Kp32 / 32);
    }
    md.w3member = w3off;
    md.Kp0 = lms[0].Kp;
    md.hidC = up16(d->hid) / kTile;
    md.outC = up16(md.out_total) / kTile;
    md.wmember = woff;
    md.bmember = boff;
    // row stride: >= widest activation, == 8 (mod 64) floats => conflict-free ds_read_b128 A fragments
    int ld = maxK;
    while (ld % 64 != 8) ld += 4;
    if (d->precision != HIPETS_PREC_F32) {
        // activation rows hold [k chunk of 32][3 pieces][32 x bf16] = 192 bytes per chunk (bf16: one piece, 64 bytes); the last layer's fp32 results share the
        // rows; a byte stride that is an ODD multiple of 16 keeps the ds_read_b128 of 16 consecutive rows on distinct slots
        int ldb = std::max(max_kc32 * 64 * pieces, lms[d->n_layers - 1].Np * 4);
        ldb = (ldb + 15) / 16 * 16;
        if ((ldb / 16) % 2 == 0) ldb += 16;
        ld = ldb / 4;
    }
    md.ld = ld;
    md.ld_in = md.Kp0;  // KSpec::WIDE instances: the model-input image's own row stride
    while (md.ld_in % 64 != 8) md.ld_in += 4;
    if (rollout_smem_bytes(kTile, md.ld, md.obs_dim, md.act_dim, md.in_dim, md.out_dim, md.out_total, 64,
                           md.propagation == HIPETS_PROP_EXPECTATION, md.lv_rows) > e->lds_max)
        return fail("model too wide for LDS (ld=%d)", md.ld);

    if (d->precision != HIPETS_PREC_F32 && e->w3pack.ensure((size_t)md.w3member * md.M * 16)) return 1;
    if (e->wpack.ensure((size_t)md.wmember * md.M * 4)) return 1;
    if (e->bpack.ensure((size_t)md.bmember * md.M * 4)) return 1;
    if (e->members.ensure((size_t)md.M * 4)) return 1;
    HCHECK(hipMemcpyAsync(e->members.p, d->members, (size_t)md.M * 4, hipMemcpyHostToDevice, st));
    // one block: the layer table, then the tables of the parametric closed forms (rollout_types.hpp form_tables), then the column table of
    // a HIPETS_OBS_COLUMNS model (obs_columns)
    static_assert(sizeof(LayerMeta) % alignof(FormTables) == 0, "FormTables follow the layer table");
    static_assert(sizeof(FormTables) % alignof(hipets_obs_column) == 0, "the column table follows the FormTables");
    const size_t forms_at = sizeof(LayerMeta) * d->n_layers, cols_at = forms_at + sizeof(FormTables), cols_bytes = cols ? sizeof(hipets_obs_column) * n_cols : 0;
    if (e->layer_meta.ensure(cols_at + cols_bytes)) return 1;
    HCHECK(hipMemcpyAsync(e->layer_meta.p, lms.data(), forms_at, hipMemcpyHostToDevice, st));
    HCHECK(hipMemcpyAsync(e->layer_meta.as<char>() + forms_at, &forms, sizeof(FormTables), hipMemcpyHostToDevice, st));
    if (cols) HCHECK(hipMemcpyAsync(e->layer_meta.as<char>() + cols_at, cols, cols_bytes, hipMemcpyHostToDevice, st));
    for (int l = 0; l < d->n_layers; ++l) {
        const float* w = reinterpret_cast<const float*>(d->weights[l]);
        const float* b = reinterpret_cast<const float*>(d->biases[l]);
        const int hidden = l < d->n_layers - 1 ? 1 : 0;
        if (pack_weights(st, e->wpack.as<float>(), w, e->members.as<int>(), md.M, Ks[l], Ns[l], lms[l].Kp, lms[l].Np, md.wmember, lms[l].woff, hidden, 0))
            return 1;
        if (d->precision != HIPETS_PREC_F32 && pack_weights_b3(st, e->w3pack.as<uint4>(), w, e->members.as<int>(), md.M, Ks[l], Ns[l], lms[l].Kp32,
                                                               lms[l].Np, md.w3member, lms[l].woff3, 0, pieces))
            return 1;
        if (pack_bias(st, e->bpack.as<float>(), b, e->members.as<int>(), md.M, Ns[l], lms[l].Np, md.bmember, lms[l].boff, hidden, 0)) return 1;
        if (lms[l].woff_pairs >= 0) {
            if (pack_weights(st, e->wpack.as<float>(), w, e->members.as<int>(), md.M, Ks[l], Ns[l], lms[l].Kp, lms[l].Np, md.wmember, lms[l].woff_pairs, 2,
                             0, d->out_dim) ||
                pack_bias(st, e->bpack.as<float>(), b, e->members.as<int>(), md.M, Ns[l], lms[l].Np, md.bmember, lms[l].boff_pairs, 2, d->out_dim))
                return 1;
        }
    }
    if (d->normalizer != HIPETS_NORM_NONE) {
        if (e->norm_mean.ensure((size_t)d->in_dim * 8) || e->norm_std.ensure((size_t)d->in_dim * 8)) return 1;
        HCHECK(hipMemcpyAsync(e->norm_mean.p, d->norm_mean, (size_t)d->in_dim * 8, hipMemcpyHostToDevice, st));
        HCHECK(hipMemcpyAsync(e->norm_std.p, d->norm_std, (size_t)d->in_dim * 8, hipMemcpyHostToDevice, st));
    }
    if (!d->deterministic) {
        const size_t nlv = (size_t)md.lv_rows * d->out_dim * 4;
        if (e->min_lv.ensure(nlv) || e->max_lv.ensure(nlv)) return 1;
        HCHECK(hipMemcpyAsync(e->min_lv.p, d->min_logvar, nlv, hipMemcpyHostToDevice, st));
        HCHECK(hipMemcpyAsync(e->max_lv.p, d->max_logvar, nlv, hipMemcpyHostToDevice, st));
    }
    std::vector<unsigned char> nd(d->obs_dim, 0);
    for (int i = 0; i < d->n_no_delta; ++i) {
        if (d->no_delta[i] < 0 || d->no_delta[i] >= d->obs_dim) return fail("no_delta index %d out of range", d->no_delta[i]);
        nd[d->no_delta[i]] = 1;
    }
    if (e->no_delta.ensure((size_t)d->obs_dim)) return 1;
    HCHECK(hipMemcpyAsync(e->no_delta.p, nd.data(), (size_t)d->obs_dim, hipMemcpyHostToDevice, st));
    HCHECK(hipStreamSynchronize(st));  // host staging buffers (nd, caller arrays) may go away after return
    md.layers = e->layer_meta.as<LayerMeta>();
    md.w3 = e->w3pack.as<uint4>();
    md.w = e->wpack.as<float>();
    md.b = e->bpack.as<float>();
    md.norm_mean = e->norm_mean.as<double>();
    md.norm_std = e->norm_std.as<double>();
    md.min_lv = e->min_lv.as<float>();
    md.max_lv = e->max_lv.as<float>();
    md.no_delta = e->no_delta.as<unsigned char>();
    e->md = md;
    e->ensemble_size = d->ensemble_size;
    e->has_model = true;
    return 0;
}

}  // namespace

extern "C" {

int hipets_set_model(hipets_engine* e, const hipets_model_desc* d, void* stream) {
    if (!e || !d) return fail("null argument");
    if (d->obs_process == HIPETS_OBS_COLUMNS) return fail("obs_process COLUMNS comes with its column table: call hipets_set_model_columns");
    return set_model(e, d, nullptr, 0, stream);
}

int hipets_set_model_columns(hipets_engine* e, const hipets_model_desc* d, const hipets_obs_column* cols, int32_t n_cols, void* stream) {
    if (!e || !d) return fail("null argument");
    if (d->obs_process != HIPETS_OBS_COLUMNS) return fail("hipets_set_model_columns: obs_process %d is not HIPETS_OBS_COLUMNS", d->obs_process);
    if (d->obs_dim < 1) return fail("bad dimensions");
    if (read_obs_columns(d, cols, n_cols)) return 1;
    return set_model(e, d, cols, n_cols, stream);
}

int hipets_planet_set_model(hipets_engine* e, const hipets_planet_desc* d, void* stream) {
    if (!e || !d) return fail("null argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    if (d->latent_size < 1 || d->action_size < 1 || d->belief_size < 1 || d->hidden_size < 1) return fail("bad PlaNet dimensions");
    const void* ptrs[] = {d->w_embed, d->b_embed, d->w_ih, d->b_ih, d->w_hh, d->b_hh, d->w_prior1, d->b_prior1,
                          d->w_prior2, d->b_prior2, d->w_rew1, d->b_rew1, d->w_rew2, d->b_rew2, d->w_rew3, d->b_rew3};
    for (const void* p : ptrs)
        if (!p) return fail("null PlaNet tensor");
    const int L = d->latent_size, A = d->action_size, Hb = d->belief_size, F = d->hidden_size;
    auto up16 = [](int x) { return (x + 15) / 16 * 16; };
    PlanetDev pd{};
    pd.latent = L; pd.action = A; pd.belief = Hb; pd.hidden = F; pd.min_std = d->min_std;
    pd.widA = up16(L + A);
    pd.widE = up16(Hb + L);
    const int widB = up16(std::max(Hb, F)), widC = up16(std::max(3 * Hb, F)), widD = up16(std::max(std::max(3 * Hb, 2 * L), 16));
    pd.segA = 0; pd.segB = pd.widA; pd.segC = pd.segB + widB; pd.segD = pd.segC + widC; pd.segE = pd.segD + widD;
    int ld = pd.segE + pd.widE;
    while (ld % 64 != 8) ld += 4;  // conflict-free ds_read_b128 A fragments (rollout.hpp header; gemm_f32.hpp lds_col)
    pd.ld = ld;
    if (planet_smem_bytes(ld) > e->lds_max) return fail("PlaNet model too wide for LDS (row of %d floats)", ld);
    // op table: K, N, source tensors, whether the output feeds another GEMM (chunk-transposed columns)
    struct OpSrc { int K, N; const void* w; const void* b; int permute; };
    const OpSrc ops[kPlanetOps] = {
        {L + A, Hb, d->w_embed, d->b_embed, 1},   {Hb, 3 * Hb, d->w_ih, d->b_ih, 0},     {Hb, 3 * Hb, d->w_hh, d->b_hh, 0},
        {Hb, F, d->w_prior1, d->b_prior1, 1},     {F, 2 * L, d->w_prior2, d->b_prior2, 0}, {Hb + L, F, d->w_rew1, d->b_rew1, 1},
        {F, F, d->w_rew2, d->b_rew2, 1},          {F, 1, d->w_rew3, d->b_rew3, 0}};
    long long woff = 0;
    int boff = 0;
    // execution order: embed, hidden gates, input gates, prior x2, reward head x3 (ops[] above is in tensor order)
    PlanetOp table[kPlanetOps];
    const int order[kPlanetOps] = {PL_EMBED, PL_GH, PL_GI, PL_PRIOR1, PL_PRIOR2, PL_REW1, PL_REW2, PL_REW3};
    const int in_off[kPlanetOps] = {pd.segA, pd.segE, pd.segB, pd.segE, pd.segB, pd.segE, pd.segB, pd.segC};
    const int out_off[kPlanetOps] = {pd.segB, pd.segD, pd.segC, pd.segB, pd.segD, pd.segB, pd.segC, pd.segD};
    const int relu[kPlanetOps] = {1, 0, 0, 1, 0, 1, 1, 0};
    const int post[kPlanetOps] = {PL_POST_NONE, PL_POST_SYNC, PL_POST_GRU, PL_POST_SYNC, PL_POST_SAMPLE, PL_POST_SYNC, PL_POST_SYNC,
                                  PL_POST_REWARD};
    for (int x = 0; x < kPlanetOps; ++x) {
        const int i = order[x];
        table[x].in_off = in_off[x];
        table[x].out_off = out_off[x];
        table[x].relu = relu[x];
        table[x].post = post[x];
        LayerMeta& lm = table[x].lm;
        lm.Kp = up16(ops[i].K);
        lm.Np = up16(ops[i].N);
        lm.woff = woff;
        lm.boff = boff;
        lm.tail_steps = (ops[i].K - (lm.Kp - 16) + 3) / 4;
        woff += (long long)lm.Kp * lm.Np;
        boff += lm.Np;
    }
    if (e->planet_w.ensure((size_t)woff * 4) || e->planet_b.ensure((size_t)boff * 4) || e->planet_member.ensure(16)) return 1;
    int* zero_member = e->planet_member.as<int>();  // the pack kernels index "member 0" of a one-member set
    HCHECK(hipMemsetAsync(zero_member, 0, 4, st));
    if (e->planet_ops.ensure(sizeof(table))) return 1;
    HCHECK(hipMemcpyAsync(e->planet_ops.p, table, sizeof(table), hipMemcpyHostToDevice, st));
    for (int x = 0; x < kPlanetOps; ++x) {
        const int i = order[x];
        const LayerMeta& lm = table[x].lm;
        if (pack_weights(st, e->planet_w.as<float>(), reinterpret_cast<const float*>(ops[i].w), zero_member, 1, ops[i].K, ops[i].N, lm.Kp, lm.Np, woff,
                         lm.woff, ops[i].permute, 1) ||
            pack_bias(st, e->planet_b.as<float>(), reinterpret_cast<const float*>(ops[i].b), zero_member, 1, ops[i].N, lm.Np, boff, lm.boff, ops[i].permute))
            return 1;
    }
    HCHECK(hipStreamSynchronize(st));  // the caller's tensors may go away after return
    pd.w = e->planet_w.as<float>();
    pd.b = e->planet_b.as<float>();
    pd.ops = e->planet_ops.as<PlanetOp>();
    e->pd = pd;
    e->planet_static = planet_static_shape(pd, table);
    e->has_planet = true;
    return 0;
}

}  // extern "C"

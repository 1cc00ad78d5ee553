/*
 * mivi.h -- C ABI of libmivi: the MI355X-native (gfx950) RepGradELBO / ADVI hot path of
 * AdvancedVI.jl v0.7.0.  extern "C", plain pointers and sizes, no exceptions across the ABI.
 *
 * Every entry point cites the reference interface it replaces (paths relative to the
 * AdvancedVI.jl repository).  The Julia-side `ccall` binding is shown in INTEGRATION.md.
 *
 * Conventions
 *   - All functions return mivi_status_t (0 = ok).  mivi_last_error(ctx) gives text.
 *   - T is float (MIVI_F32) or double (MIVI_F64), fixed per context.
 *   - `*_dev` pointers are device (HBM) pointers valid on the context's device; calls taking
 *     only device pointers are ASYNCHRONOUS on the context's stream (no host sync).
 *     `*_host` convenience variants copy in/out and synchronise.
 *   - Sample layout: d x M column-major, one sample per column (src/utils.jl:6 `eachsample=eachcol`).
 *   - Parameter layout (what `Optimisers.destructure(q)` yields):
 *       mean-field: [location (d); diag(scale) (d)]                 src/families/location_scale.jl:39-43
 *       full-rank : [location (d); vec(scale) column-major (d*d)]   src/families/location_scale.jl:21
 *                   entries above the diagonal are ignored on input (LowerTriangular) and the
 *                   gradient written there is exactly 0.
 *       low-rank  : [location (d); scale_diag (d); vec(scale_factors) column-major (d*rank)]
 *                   src/families/location_scale_low_rank.jl:22-41 (the functor's field order)
 *   - The objective value is the NEGATIVE ELBO (src/algorithms/repgradelbo.jl:117,148).
 *   - Randomness is explicit: eps is a pure function of (seed, estimate_idx, global sample m, i)
 *     through Philox4x32-10 + Box-Muller (csrc/philox.h), replacing the mutable `rng` threaded
 *     through src/algorithms/repgradelbo.jl:104-110.  One estimate consumes one estimate_idx.
 *     Low-rank family: the draws of an estimate are ONE stream of d + rank rows per column (i runs over d + rank, the Philox block
 *     index is m * ceil((d + rank)/4) + i/4); rows 0 .. d-1 are u1 (the diagonal part), rows d .. d+rank-1 are u2 (the factors' part).
 *   - A context is single-owner (like the reference's rng); distinct contexts are independent.
 */
#ifndef MIVI_H
#define MIVI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIVI_VERSION_MAJOR 0
#define MIVI_VERSION_MINOR 1

typedef int32_t mivi_status_t;
enum {
  MIVI_OK = 0,
  MIVI_ERR_BAD_ARG = 1,
  MIVI_ERR_NONFINITE = 2,      /* objective not finite: host maps to the ErrorException of src/algorithms/common.jl:83-89 */
  MIVI_ERR_NONPOSITIVE_SCALE = 3, /* log of a non-positive scale diagonal: the DomainError ClipScale exists to prevent */
  MIVI_ERR_HIP = 4,
  MIVI_ERR_NO_TARGET = 5,
  MIVI_ERR_UNSUPPORTED = 6
};

typedef enum { MIVI_F32 = 0, MIVI_F64 = 1 } mivi_dtype_t;

/* MeanFieldGaussian / FullRankGaussian: src/families/location_scale.jl:139-141 / :124-128;
 * LowRankGaussian: src/families/location_scale_low_rank.jl:140-145 -- z = scale_diag .* u1 + scale_factors * u2 + location, rank =
 * cfg.rank columns of factors.  What family 2 supports: create / destroy / synchronize / set_stream / params_len, every mivi_set_target_*
 * and mivi_set_bijector_stacked, mivi_sample (eps_dev: T[(d + rank) * n_mc]), mivi_logpdf[_host] (std NULL), mivi_estimate_gradient[_host / _n / _each] (the batched
 * forms as sequential single calls), mivi_estimate_objective[_host], mivi_clip_scale / _descent_update / _adam_update / _cocob_update /
 * the DoG entries, and mivi_optimize_steps / _loop as a graph of launches (op 0 or 1).  Every other entry that reads parameters returns
 * MIVI_ERR_UNSUPPORTED on it (the score-gradient and measure-space entries, partials / finalize / dist / p2p, the profile entries,
 * mivi_prox_scale_entropy and op = 2: the reference has no ProximalLocationScaleEntropy method for the family). */
typedef enum { MIVI_MEANFIELD = 0, MIVI_FULLRANK = 1, MIVI_LOWRANK = 2, MIVI_REALNVP = 3, MIVI_NSF = 4 } mivi_family_t;
#define MIVI_LOWRANK_MAX_RANK 64

/* MIVI_REALNVP: the RealNVP normalizing flow of docs/src/tutorials/flows.md (Dinh et al.; the masks and activations of
 * NormalizingFlows.realnvp), created by mivi_create_flow.  All index sets are 0-based.
 *   base     eps ~ N(0, I_d): the mean-field family's Philox stream, d rows.  No parameters.
 *   layers   l = 1 .. n_layers, x^0 = eps, z = x^L.  A_l = {0, 2, 4, ...} for odd l, {1, 3, 5, ...} for even l, B_l the rest;
 *            c = x^{l-1}[B_l], a = x^{l-1}[A_l];  x^l[B_l] = c,  x^l[A_l] = a .* exp(s_l(c)) + t_l(c)
 *   nets     each |B_l| -> hidden[0] -> ... -> hidden[n_hidden - 1] -> |A_l|; hidden layers leakyrelu(W_j . + b_j) with slope 0.01, the
 *            output W . + b; s_l applies tanh to it, t_l nothing
 *   log q    log q(z) = -1/2 |eps|^2 - d/2 log 2 pi - sum_l 1' s_l(c_l) at eps = T^-1(z); inverse layer: a = (y_A - t(c)) .* exp(-s(c))
 *   params   for l = 1 .. L: the s net, then the t net; a net is [vec W_1 (column-major, out x in); b_1; ...; vec W_{H+1}; b_{H+1}]
 *   limits   2 <= d <= 128, 1 <= hidden[j] <= 64, 1 <= n_hidden <= 3, 1 <= n_layers <= 32, any n_mc >= 1
 *   entropy  MIVI_ENT_MONTE_CARLO and MIVI_ENT_STL: value = mean[-ell(z_m) + log q(z_m)] for both (ell includes the bijector's
 *            logabsdetjac); the others need entropy(q), which a flow does not have: MIVI_ERR_UNSUPPORTED
 * What family 3 supports: destroy / synchronize / set_stream / params_len, every mivi_set_target_* and mivi_set_bijector_stacked[_ex],
 * mivi_sample (eps_dev: T[d * n_mc]) / mivi_sample_constrained, mivi_logpdf[_host] (std NULL) / mivi_logpdf_constrained[_host],
 * mivi_estimate_gradient[_host / _n / _each] (the batched forms as sequential single calls), mivi_estimate_objective[_host], the update
 * entries without a scale (descent / adam / cocob / DoG), and mivi_optimize_steps / _loop as a graph of launches with op 0 (op 1 and 2:
 * MIVI_ERR_UNSUPPORTED -- ClipScale and the proximal operator have no method for a family without a scale; mivi_clip_scale likewise).
 * mivi_set_base_dist accepts MIVI_BASE_NORMAL, which changes nothing, and refuses every other base.  Every other entry that reads
 * parameters returns MIVI_ERR_UNSUPPORTED on it with a message naming the entry and the family: what the low-rank family is refused on,
 * and the batch schedule (mivi_logreg_set_batch_schedule / _seek_batch, mivi_optimize_loop_batches), which the low-rank family has. */
#define MIVI_FLOW_MAX_D 128
#define MIVI_FLOW_MAX_HIDDEN 64
#define MIVI_FLOW_MAX_LAYERS 32
typedef struct {
  int32_t n_layers;   /* L, 1 .. MIVI_FLOW_MAX_LAYERS */
  int32_t n_hidden;   /* H, 1 .. 3 hidden layers per net */
  int32_t hidden[3];  /* their widths, 1 .. MIVI_FLOW_MAX_HIDDEN (entries from n_hidden on are not read) */
} mivi_flow_t;

/* MIVI_NSF: the neural spline flow (Durkan et al., 2019; the coupling flow `nsf` of NormalizingFlows.jl beside `realnvp`), created by
 * mivi_create_spline_flow.  RealNVP's affine map of each coupling layer is replaced by a monotone rational-quadratic spline on [-B, B]
 * with K bins, in the form Bijectors.RationalQuadraticSpline documents (no minimum bin size or slope).  All index sets are 0-based.
 *   base     eps ~ N(0, I_d): the mean-field family's Philox stream, d rows.  No parameters.
 *   layers   l = 1 .. n_layers, x^0 = eps, z = x^L.  A_l = {0, 2, 4, ...} for odd l, {1, 3, 5, ...} for even l, B_l the rest (RealNVP's);
 *            c = x^{l-1}[B_l] passes through, x^l[A_l][i] = f(a_i; theta_i(c)) with a = x^{l-1}[A_l]
 *   net      ONE per layer, |B_l| -> hidden[0] -> ... -> hidden[n_hidden - 1] -> |A_l| (3K - 1); hidden layers leakyrelu(W_j . + b_j) with
 *            slope 0.01, the output layer W . + b (nothing applied).  Output rows are coordinate-major: coordinate i of A_l (its i-th
 *            member) owns the rows i (3K - 1) ... i (3K - 1) + 3K - 2 = theta_i, in the order u^w_1..K, u^h_1..K, u^d_1..K-1
 *   spline   of one coordinate, from theta = (u^w, u^h, u^d):  w = 2B softmax(u^w), h = 2B softmax(u^h); knots X_0 = -B,
 *            X_k = X_{k-1} + w_k, Y_0 = -B, Y_k = Y_{k-1} + h_k; slopes delta_0 = delta_K = 1, delta_k = softplus(u^d_k) = log(1 + exp u^d_k).
 *            a <= -B or a >= B:  f(a) = a, log f'(a) = 0 (the identity tails).
 *            otherwise bin k is the one with X_{k-1} <= a < X_k (a >= X_{K-1}: bin K), and with xi = (a - X_{k-1}) / w_k, s = h_k / w_k,
 *            D = s + (delta_k + delta_{k-1} - 2s) xi (1 - xi):
 *              f(a)      = Y_{k-1} + h_k (s xi^2 + delta_{k-1} xi (1 - xi)) / D
 *              log f'(a) = 2 log s + log(delta_k xi^2 + 2 s xi (1 - xi) + delta_{k-1} (1 - xi)^2) - 2 log D
 *   inverse  y <= -B or y >= B: a = y.  Otherwise bin k with Y_{k-1} <= y < Y_k, dy = y - Y_{k-1}, t = delta_k + delta_{k-1} - 2s,
 *            qa = h_k (s - delta_{k-1}) + dy t, qb = h_k delta_{k-1} - dy t, qc = -s dy, xi = 2 qc / (-qb - sqrt(qb^2 - 4 qa qc)),
 *            a = X_{k-1} + xi w_k
 *   log q    log q(z) = -1/2 |eps|^2 - d/2 log 2 pi - sum_l sum_{i in A_l} log f'_{l,i}(a_{l,i}) at eps = T^-1(z)
 *   params   for l = 1 .. L the layer's net [vec W_1 (column-major, out x in); b_1; ...; vec W_{H+1}; b_{H+1}], as a RealNVP net lies
 *   limits   2 <= d <= 128, 1 <= hidden[j] <= 64, 1 <= n_hidden <= 3, 1 <= n_layers <= 32, 2 <= n_bins <= 16, bound > 0 and finite,
 *            any n_mc >= 1, f32 and f64
 *   entropy  as MIVI_REALNVP: MIVI_ENT_MONTE_CARLO and MIVI_ENT_STL
 * Family 4 supports exactly the entries family 3 supports (the list above) and is refused, with a message naming the entry and "neural
 * spline flow family (MIVI_NSF)", on exactly the entries family 3 is refused on.
 * NormalizingFlows.nsf's own parameter order (its Flux conditioner's layout and its minimum bin sizes, if it sets any) is NOT what this
 * header fixes: binding it belongs to julia/MIVI.jl, is not part of the library and has not been checked against that package. */
#define MIVI_NSF_MAX_BINS 16
typedef struct {
  int32_t n_layers;   /* L, 1 .. MIVI_FLOW_MAX_LAYERS */
  int32_t n_hidden;   /* H, 1 .. 3 hidden layers of the conditioner */
  int32_t hidden[3];  /* their widths, 1 .. MIVI_FLOW_MAX_HIDDEN (entries from n_hidden on are not read) */
  int32_t n_bins;     /* K, 2 .. MIVI_NSF_MAX_BINS */
  double bound;       /* B > 0, finite */
} mivi_spline_flow_t;

/* src/algorithms/entropy.jl: ClosedFormEntropy :25-29, ClosedFormEntropyZeroGradient :11-15,
 * MonteCarloEntropy :40-46, StickingTheLandingEntropy :57-65, StickingTheLandingEntropyZeroGradient :78-90 */
typedef enum {
  MIVI_ENT_CLOSED_FORM = 0,
  MIVI_ENT_CLOSED_FORM_ZERO_GRAD = 1,
  MIVI_ENT_MONTE_CARLO = 2,
  MIVI_ENT_STL = 3,
  MIVI_ENT_STL_ZERO_GRAD = 4
} mivi_entropy_t;

/* RepGradELBO(n_samples; entropy) + family + RNG key: src/algorithms/repgradelbo.jl:21-24,72-74 */
typedef struct {
  int32_t dtype;      /* mivi_dtype_t */
  int32_t family;     /* mivi_family_t */
  int32_t d;          /* LogDensityProblems.dimension(prob) */
  int32_t n_mc;       /* samples THIS context draws per estimate (RepGradELBO.n_samples / world size) */
  int32_t entropy;    /* mivi_entropy_t */
  int32_t device;     /* HIP device ordinal */
  uint64_t seed;      /* Philox key */
  int32_t m_offset;   /* first GLOBAL sample index owned by this context (multi-GPU shard); 0 on one GPU */
  int32_t m_total;    /* GLOBAL n_samples the estimate is normalised by; 0 => n_mc */
  void *stream;       /* hipStream_t to launch on; NULL = the HIP null (legacy default) stream */
  int32_t own_stream; /* != 0: ignore `stream` and create a non-blocking stream owned by the context */
  int32_t rank;       /* MIVI_LOWRANK only: columns of scale_factors, 1 .. MIVI_LOWRANK_MAX_RANK (not read for the other families) */
} mivi_config_t;

typedef struct mivi_ctx mivi_ctx_t;

/* ---- lifetime ------------------------------------------------------------------------------- */
/* replaces AdvancedVI.init(rng, obj::RepGradELBO, adtype, q, prob, params, restructure)
 * (src/algorithms/repgradelbo.jl:41-70): one-time preparation, no AD to prepare.
 * MIVI_LOWRANK: MIVI_ERR_BAD_ARG unless 1 <= rank <= MIVI_LOWRANK_MAX_RANK; MIVI_ERR_UNSUPPORTED for a sharded context (m_offset != 0 or
 * m_total not in {0, n_mc}). */
mivi_status_t mivi_create(const mivi_config_t *cfg, mivi_ctx_t **out);
/* A MIVI_REALNVP context (cfg->family must be MIVI_REALNVP; mivi_create answers MIVI_ERR_BAD_ARG for that family).  MIVI_ERR_BAD_ARG
 * outside the limits above; MIVI_ERR_UNSUPPORTED for an entropy kind other than MIVI_ENT_MONTE_CARLO / MIVI_ENT_STL and for a sharded
 * context (m_offset != 0 or m_total not in {0, n_mc}). */
mivi_status_t mivi_create_flow(const mivi_config_t *cfg, const mivi_flow_t *flow, mivi_ctx_t **out);
/* A MIVI_NSF context (cfg->family must be MIVI_NSF; mivi_create and mivi_create_flow answer MIVI_ERR_BAD_ARG for that family).  The
 * same answers as mivi_create_flow: MIVI_ERR_BAD_ARG outside the limits above, MIVI_ERR_UNSUPPORTED for the entropy kind and the shard. */
mivi_status_t mivi_create_spline_flow(const mivi_config_t *cfg, const mivi_spline_flow_t *flow, mivi_ctx_t **out);
mivi_status_t mivi_destroy(mivi_ctx_t *ctx);
const char *mivi_last_error(const mivi_ctx_t *ctx);
int32_t mivi_version(void);
mivi_status_t mivi_set_stream(mivi_ctx_t *ctx, void *hip_stream);
/* Wait for the context's stream.  Device entries never synchronise; a non-finite objective or a non-positive scale
 * diagonal is recorded in a sticky device flag which this call (and the _host entries / mivi_optimize_steps) reads and
 * clears, returning MIVI_ERR_NONFINITE / MIVI_ERR_NONPOSITIVE_SCALE -- the once-per-step isfinite check of
 * src/algorithms/common.jl:83-89. */
mivi_status_t mivi_synchronize(mivi_ctx_t *ctx);
/* length of `params` / gradient: 2d or d + d*d  (test/families/location_scale.jl:146-155); low-rank: 2d + d*rank */
int64_t mivi_params_len(const mivi_ctx_t *ctx);
/* length of the shard-additive partials buffer ([sum_m W (d); sum_m W (x) eps; sum ell; sum 0.5|eps|^2]):
 * mean-field 2d + 2; full-rank d + d(d+1)/2 + 2 -- only the lower triangle travels, packed column by column
 * (entry (i, j), j <= i, at d + j*d - j(j-1)/2 + (i - j)) so the all-reduce moves half the bytes of the gradient.
 * Low-rank family: 0 (no sharded estimates). */
int64_t mivi_partials_len(const mivi_ctx_t *ctx);

/* ---- the base distribution of the location-scale families ----------------------------------- *
 * MvLocationScale(location, scale, dist): src/families/location_scale.jl:15-19, docs/src/families.md:72-101 -- z = C u + m with the
 * entries of u i.i.d. from a univariate base phi: Normal() (the default), Laplace() or TDist(nu).
 * nu: degrees of freedom, read for MIVI_BASE_TDIST only (nu > 0, any real).
 * The draws stay a pure function of (seed, estimate_idx, global column m, row i), key and counter as for the normal stream (philox.h):
 *   Laplace: element (i, m) takes word i % 4 of block q = m * ceil(d/4) + i/4; sign + if the word's top bit is set; magnitude -ln v,
 *            v = (((w >> 8) & 0x7fffff) + 0.5) 2^-23 (f32 contexts), v = ((w & 0x7fffffff) + 0.5) 2^-31 (f64 contexts).
 *   TDist  : Bailey's polar form T = sqrt(nu expm1(-(2/nu) ln U)) cos(2 pi V); element (i, m) takes words 2 (i % 2) (-> U) and
 *            2 (i % 2) + 1 (-> V) of block q = m * ceil(d/2) + i/2; word -> uniform as Box-Muller: ((w >> 9) + 0.5) 2^-23 (f32),
 *            (w + 0.5) 2^-32 (f64).
 * MIVI_BASE_NORMAL is a no-op in effect: such a context gives bitwise the results of one that never called this, on every route.
 * MIVI_ERR_BAD_ARG: an unknown base, nu <= 0 or not finite.  MIVI_ERR_UNSUPPORTED for a non-normal base on a MIVI_LOWRANK context or a
 * sharded one (m_offset != 0 or m_total not in {0, n_mc}).  Invalidates captured graphs, like mivi_set_target_*.
 * What a non-normal base supports (both families, both precisions): mivi_sample, mivi_logpdf[_host], mivi_estimate_gradient[_host / _n / _each] (the batched
 * forms as sequential single calls, bitwise equal to them), mivi_estimate_objective[_host] (any n_samples, all five entropy kinds), every
 * mivi_set_target_* incl. the gradient callback, mivi_set_bijector_stacked, the update entries (clip, descent, adam, cocob, DoG / DoWG,
 * mivi_prox_scale_entropy, mivi_axpby) and mivi_optimize_steps / _loop as the graph of launches with every rule, operator and averager.
 * Every other entry that reads parameters returns MIVI_ERR_UNSUPPORTED with a message naming the base, before it reads a buffer: the
 * score-gradient entries, mivi_gauss_expected_grad_hess*, the natgrad / sqrt-ngd / bam / wass entries (Gaussian by definition),
 * partials / finalize / dist / comm / p2p, the profile entries. */
typedef enum { MIVI_BASE_NORMAL = 0, MIVI_BASE_LAPLACE = 1, MIVI_BASE_TDIST = 2 } mivi_base_t;
mivi_status_t mivi_set_base_dist(mivi_ctx_t *ctx, int32_t base, double nu);

/* ---- targets: the LogDensityProblems plugin seam --------------------------------------------- *
 * replaces LogDensityProblems.logdensity / logdensity_and_gradient / dimension as called from
 * src/algorithms/repgradelbo.jl:84-86 and src/mixedad_logdensity.jl:23-34.  Built-in targets run
 * fused on the device; the callback target is the generic plugin route (batched over columns). */

/* MvNormal(mean, Diagonal(std.^2)): test/models/normal.jl:56-75, bench/benchmarks.jl:43-47. host ptrs, T[d]. */
mivi_status_t mivi_set_target_diag_gauss(mivi_ctx_t *ctx, const void *mean_host, const void *std_host);
/* MvNormal(mean, L*L'): test/models/normal.jl:36-54.  host ptrs: mean T[d], L T[d*d] column-major lower. */
mivi_status_t mivi_set_target_dense_gauss(mivi_ctx_t *ctx, const void *mean_host, const void *chol_L_host);
/* Hierarchical logistic regression over theta = [beta (d-1); s]:
 *   variant 0: docs/src/tutorials/subsampling.md:26-38 (s = log sigma, Normal(0,3) prior on sigma, likeadj = n_data/n)
 *   variant 1: README.md:42-66 under the exp-bijector wrapper README.md:91-106 (LogNormal(0,3) prior, + log|det J| = s)
 * X: n x (d-1) COLUMN-major T (X[r + k*n], Julia's native Matrix layout), y: n bytes {0,1}.  x_on_device != 0 => X,y are device ptrs
 * (borrowed, must outlive the ctx); otherwise host ptrs, copied. */
mivi_status_t mivi_set_target_logreg(mivi_ctx_t *ctx, const void *X, const uint8_t *y, int64_t n,
                                     int32_t variant, double likeadj, int32_t x_on_device);
/* AdvancedVI.subsample(prob, batch) for the built-in logistic regression (docs/src/tutorials/subsampling.md:99-102,
 * src/algorithms/subsampledobjective.jl:85-87): the data set given to mivi_set_target_logreg stays resident, the target
 * becomes its rows idx_host[0..b) (0-based) with the likelihood scaled by `likeadj` (= n_data / b, subsampling.md:37).
 * b = 0 restores the full data set.  Synchronises the stream (the batch buffers are reused from step to step). */
mivi_status_t mivi_logreg_select_rows(mivi_ctx_t *ctx, const int64_t *idx_host, int64_t b, double likeadj);

/* A schedule of minibatches resident on the device: what ReshufflingBatchSubsampling delivers to estimate_gradient! over a run of steps
 * (src/reshuffling.jl:38-60 with drop_trailing_batch_if_too_small: every batch has `batch` rows), uploaded once per chunk of steps.  While one
 * is set every estimate entry (mivi_estimate_gradient[_host/_n/_each], mivi_estimate_objective[_host], mivi_optimize_steps / _loop) evaluates
 * the SELECTED batch -- its rows are read out of the resident data set through the schedule, nothing is gathered ahead of the estimate and
 * no host round trip is made per step; mivi_optimize_loop_batches walks the batches, one per step.
 *   kernels  0 by size | 1 the fused minibatch kernel (one workgroup per slab of batch rows, rows and residuals in LDS: the target is two
 *            launches; where not even a minimal slab fits the LDS -- p beyond a few thousand -- it is 2) | 2 a device gather of the batch
 *            and the kernels of the resident data set on the copy (bitwise what mivi_logreg_select_rows + the estimate give)
 * Every index is checked on the host before anything is uploaded: MIVI_ERR_BAD_ARG for a row outside the data set, batch < 1, likeadj <= 0;
 * MIVI_ERR_NO_TARGET without a logistic regression; a failed call leaves the previous selection in force.  Repeated rows are allowed.
 * After the call the target is batch 0.  The schedule and mivi_logreg_select_rows replace each other; n_batches = 0 (like select_rows with
 * b = 0) restores the full data set.  The buffers grow but do not move when a schedule of the same or a smaller size replaces one, and a
 * schedule of the same batch size, kernels and likeadj keeps a recorded loop: a chunked driver records once.  May synchronise the stream.
 * The other entries that read the data set (mivi_gauss_expected_grad_hess*, the measure-space updates and steps, the score-gradient,
 * partials / sharded / peer-to-peer and profile entries) return MIVI_ERR_UNSUPPORTED on a scheduled context: their host-driven drivers
 * select rows with mivi_logreg_select_rows. */
typedef struct mivi_batch_schedule {
  const int64_t *rows_host;          /* int64[n_batches * batch], batch-major, 0-based rows of the data set given to mivi_set_target_logreg */
  const uint64_t *estimate_idx_host; /* uint64[n_batches] or NULL: the estimate index mivi_optimize_loop_batches uses for each batch */
  int64_t batch;                     /* rows per batch, >= 1 */
  int32_t n_batches;                 /* 0 removes the schedule: back to the full data set */
  int32_t kernels;                   /* 0 | 1 | 2, above */
  double likeadj;                    /* n_data / batch (subsampling.md:37), > 0 */
} mivi_batch_schedule_t;
mivi_status_t mivi_logreg_set_batch_schedule(mivi_ctx_t *ctx, const mivi_batch_schedule_t *sched);
/* The target becomes batch k of the schedule, 0 <= k < n_batches (MIVI_ERR_BAD_ARG otherwise, the selection unchanged).  A host-side
 * selection: no device work, no synchronisation; captured graphs are invalidated as by mivi_logreg_select_rows. */
mivi_status_t mivi_logreg_seek_batch(mivi_ctx_t *ctx, int32_t k);

/* Neal's funnel on the constrained scale + Stacked([log, identity]) bijector (README.md:76-82,102-106):
 * theta_1 = exp(eta_1) ~ LogNormal(0, sigma_v), theta_i ~ Normal(0, theta_1), log|det J| = eta_1. */
mivi_status_t mivi_set_target_funnel(mivi_ctx_t *ctx, double sigma_v);

/* The same funnel WITHOUT the built-in bijector: theta = [s; x] on the constrained scale (s > 0), log p = log LogNormal(s; 0,
 * sigma_v) + sum_i log Normal(x_i; 0, s).  Compose it with mivi_set_bijector_stacked({exp on [0,1), identity on [1,d)}) to obtain
 * the target of mivi_set_target_funnel (tests/test_gpu_bijector.py pins the two against each other). */
mivi_status_t mivi_set_target_funnel_constrained(mivi_ctx_t *ctx, double sigma_v);

/* Bijectors.Stacked over index blocks, wrapping WHATEVER target is set (README.md:76-82,91-119,
 * docs/src/tutorials/constrained.md:154-196: `TransformedLogDensityProblem(prob, binv)`):
 *   logdensity(eta) = log pi(binv(eta)) + logabsdetjac(binv, eta),  binv = identity or exp per block.
 * ranges_host[2 b], ranges_host[2 b + 1] = [begin, end) of block b (0-based, disjoint, inside [0, d)); kinds_host[b]: 0 identity,
 * 1 exp.  Coordinates in no block are identity.  n_blocks = 0 removes the bijector.  The variational family stays on the
 * unconstrained scale; the target (built-in or plugin callback) sees constrained samples binv(z), its gradient g comes back as
 * J' g + d logabsdetjac / d eta  (exp block: x_i g_i + 1), its value gains sum over exp coordinates of eta_i.
 * With a bijector the estimate runs on the explicit-sample route (Z materialised, transformed in place). */
mivi_status_t mivi_set_bijector_stacked(mivi_ctx_t *ctx, int32_t n_blocks, const int32_t *ranges_host, const int32_t *kinds_host);

/* The same with bounded and ordered blocks: the maps Bijectors.jl attaches to Uniform / Beta / truncated supports, to half-bounded
 * parameters with a non-zero bound and to ordered vectors (cut-points, mixture locations).  kinds_host[b] is a mivi_bijector_kind_t:
 *   MIVI_BIJ_TRUNCATED  one pair (lb, ub) = bounds_host[2 b], bounds_host[2 b + 1] per block; +-INFINITY means "no bound"
 *       both finite : s = sigma(eta), x = lb + (ub - lb) s, ladj = log(ub - lb) - |eta| - 2 log1p(e^-|eta|),
 *                     d/d eta = (ub - lb) s (1 - s) g + (1 - 2 s)
 *       lb only     : x = lb + e^eta, ladj = eta, d/d eta =  e^eta g + 1        (lb = 0: bitwise MIVI_BIJ_EXP)
 *       ub only     : x = ub - e^eta, ladj = eta, d/d eta = -e^eta g + 1
 *       neither     : identity
 *   MIVI_BIJ_ORDERED    the block [b, e) maps to a strictly increasing vector: x_b = eta_b, x_k = x_{k-1} + e^eta_k, ladj = sum_{k>b} eta_k;
 *                       with S_k = sum_{j=k}^{e-1} g_j: d/d eta_b = S_b, d/d eta_k = e^eta_k S_k + 1.  A block of length 1 is identity.
 * (g = grad_x log pi(x), ladj = the block's part of logabsdetjac(binv, eta) per sample.)  bounds_host: double[2 n_blocks], read for
 * MIVI_BIJ_TRUNCATED blocks only; may be NULL when there is none.  One workgroup per sample column, the ordered kind as a segmented scan
 * in f64; the backward pass takes e^eta and sigma(eta) from a saved copy of eta (d x n_mc, allocated only when such a block is present),
 * never from differences of the stored x, which cancel in f32 next to a large bound.  In f32 a two-sided block saturates to x = lb or
 * x = ub for |eta| beyond ~17 (a target that is finite there keeps value and gradient finite); ladj never evaluates log sigma of a
 * saturated sigma.  Every route mivi_set_bijector_stacked serves takes the new kinds; the refusals behind a bijector (the second-order
 * branch, FisherMinBatchMatch, the fused / launch-free routes) are the same.  A list of identity / exp blocks alone (truncated(-inf, +inf)
 * and one-coordinate ordered blocks are identity) is exactly mivi_set_bijector_stacked.  Dimension-changing maps (simplex, correlation /
 * covariance Cholesky) are out of scope: target and family share one d.
 * MIVI_ERR_BAD_ARG with a message: a NaN bound, lb >= ub, a kind outside 0 .. 3, a range outside [0, d), overlapping blocks; the bijector
 * that was set stays.  MIVI_ERR_HIP (the tables could not be placed on the device): the context is left with NO bijector. */
typedef enum { MIVI_BIJ_IDENTITY = 0, MIVI_BIJ_EXP = 1, MIVI_BIJ_TRUNCATED = 2, MIVI_BIJ_ORDERED = 3 } mivi_bijector_kind_t;
mivi_status_t mivi_set_bijector_stacked_ex(mivi_ctx_t *ctx, int32_t n_blocks, const int32_t *ranges_host, const int32_t *kinds_host,
                                           const double *bounds_host);

/* Generic plugin: batched `logdensity_and_gradient` (src/mixedad_logdensity.jl:28) over the columns of Z.
 * Called on the host thread inside mivi_estimate_* with HOST buffers: Z (d x M col-major) in,
 * ell (M) and G (d x M) out.  Return non-zero to abort (-> MIVI_ERR_BAD_ARG). */
typedef int32_t (*mivi_logdensity_and_gradient_fn)(void *user, const void *Z_host, int32_t d, int32_t M,
                                                   void *ell_host, void *G_host);
/* value-only plugin (LogDensityProblems.logdensity), used by mivi_estimate_objective when set; may be NULL */
typedef int32_t (*mivi_logdensity_fn)(void *user, const void *Z_host, int32_t d, int32_t M, void *ell_host);
mivi_status_t mivi_set_target_callback(mivi_ctx_t *ctx, mivi_logdensity_and_gradient_fn fn_grad,
                                       mivi_logdensity_fn fn_value, void *user);

/* A target that has ONLY a batched `logdensity` (LogDensityProblems.LogDensityOrder{0}(): not differentiable, or no gradient at hand) --
 * what the score-gradient estimator is for (src/algorithms/scoregradelbo.jl:44,108 evaluates nothing but `logdensity`).  The score
 * entries and mivi_estimate_objective accept it; every entry that needs the target's gradient returns MIVI_ERR_UNSUPPORTED on it.
 * fn_value must not be NULL (mivi_set_target_callback keeps rejecting a NULL gradient function). */
mivi_status_t mivi_set_target_value_callback(mivi_ctx_t *ctx, mivi_logdensity_fn fn_value, void *user);

/* ---- the hot path ----------------------------------------------------------------------------- */
/* rand(rng, q, n_mc): src/families/location_scale.jl:71-87 (exposes the sample kernel for parity).
 * Z_dev: T[d*n_mc]; eps_dev: T[d*n_mc] or NULL.  Low-rank family (location_scale_low_rank.jl:66-100): eps_dev is T[(d + rank)*n_mc],
 * column m = (u1 (d); u2 (rank)) of sample m. */
mivi_status_t mivi_sample(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx,
                          void *Z_dev, void *eps_dev);

/* Distributions.logpdf(q, z) for the n columns of Z, points the CALLER supplies: src/families/location_scale.jl:59-63,
 * src/families/location_scale_low_rank.jl:45-68 (checked by test/families/location_scale.jl:38-42, location_scale_low_rank.jl:37-46).
 *   Z_dev    T[d*n], d x n column-major with leading dimension d -- the layout mivi_sample writes.  n >= 1 is independent of cfg.n_mc
 *            (columns are walked 16384 at a time); n > 2^31 - 16385: MIVI_ERR_BAD_ARG.
 *   logq_dev T[n] <- logq[k] = sum_i log phi(u_ik) - log det C with u_k = C^-1 (z_k - mu) and phi the context's base (mivi_set_base_dist:
 *            Normal, Laplace, TDist(nu)); the sums over i are accumulated in f64.  Low-rank family (Gaussian only): the Woodbury form
 *            -d/2 log 2 pi - sum log D - 1/2 logdet(I + U' D^-2 U) - 1/2 (|t|^2 - s' (I + U' D^-2 U)^-1 s), t = D^-1 (z - m), s = U' D^-1 t.
 *   std_dev  T[d*n] or NULL <- u, the standardised points (the residuals of z under q), same layout as Z.  The low-rank family has no
 *            square scale to standardise by: a non-NULL std_dev returns MIVI_ERR_UNSUPPORTED there, before any buffer is read.
 * Mean-field: one streaming kernel.  Full-rank: a forward block substitution C X = Z - mu on the matrix cores
 * (kernels_logpdf.hip: f32 operands, exact products, every sum and X itself in f64), for EVERY d mivi_create admits -- X stays in LDS
 * while 16 columns of it fit and in an f64 scratch of min(n, 16384) columns past that; there is no size at which the entry refuses.
 * q lives on the unconstrained scale: a Stacked bijector (mivi_set_bijector_stacked) wraps the TARGET and is ignored here, and no
 * target is needed.  Allowed on sharded contexts (nothing of the estimate's sample axis is involved).  Asynchronous on the context's
 * stream.  The call works in scratch of its own and leaves the context as it found it: cached graphs stay valid, the eps speculation
 * and every estimate buffer are untouched, so the estimates before and after it are bitwise those of a context that never called it.
 * MIVI_ERR_BAD_ARG: params_dev, Z_dev or logq_dev NULL; n < 1.  A scale diagonal that is not positive sets the sticky device flag
 * (MIVI_ERR_NONPOSITIVE_SCALE from mivi_synchronize), like the estimates.  A non-finite point gives a non-finite logq[k] for that column
 * only and sets no flag: it is the caller's data, not the iterate's state. */
mivi_status_t mivi_logpdf(mivi_ctx_t *ctx, const void *params_dev, const void *Z_dev, int64_t n, void *logq_dev, void *std_dev);
/* Same, host buffers, synchronous; returns MIVI_ERR_NONPOSITIVE_SCALE itself. */
mivi_status_t mivi_logpdf_host(mivi_ctx_t *ctx, const void *params_host, const void *Z_host, int64_t n, void *logq_host, void *std_host);

/* Bijectors.TransformedDistribution(q, binv) with the Stacked bijector that is set (docs/src/tutorials/basic.md:210-247,
 * constrained.md:228-231): the constrained approximation people sample from and score.  Every family and base mivi_sample / mivi_logpdf serve.
 *
 * mivi_sample_constrained: X_dev T[d*n_mc] <- binv(z), z the draws mivi_sample returns for estimate_idx; eta_dev T[d*n_mc] or NULL <- z itself.
 * No bijector: X = z.
 *
 * mivi_logpdf_constrained: logq[k] = log q(b(x_k)) - logabsdetjac(binv, b(x_k)) at the caller's CONSTRAINED points X (d x n, the layout of
 * mivi_logpdf).  An inverse-direction kernel (truncated: u = (x - lb) / (ub - lb), eta = log u - log1p(-u), or log(x - lb) / log(ub - x);
 * ordered: eta_k = log(x_k - x_{k-1}); everything in f64, rounded once) runs in front of mivi_logpdf, in scratch of its own: the same
 * "leaves the context as it found it" contract.  A finite point outside the support -- on or beyond a bound, a non-increasing ordered
 * block -- gives exactly -inf for that column, a NaN point gives NaN for that column only; neither sets a status flag.  No bijector:
 * mivi_logpdf. */
mivi_status_t mivi_sample_constrained(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx, void *X_dev, void *eta_dev);
mivi_status_t mivi_logpdf_constrained(mivi_ctx_t *ctx, const void *params_dev, const void *X_dev, int64_t n, void *logq_dev);
/* Same, host buffers, synchronous. */
mivi_status_t mivi_logpdf_constrained_host(mivi_ctx_t *ctx, const void *params_host, const void *X_host, int64_t n, void *logq_host);

/* estimate_gradient!(rng, obj::RepGradELBO, adtype, out, state, params, restructure):
 * src/algorithms/repgradelbo.jl:151-177 (+ the AD shim src/AdvancedVI.jl:57-67 it replaces).
 * value_dev: T[1] <- -elbo; grad_dev: T[params_len] fully overwritten. Asynchronous for built-in
 * targets; synchronous (host round trip) for the callback target. */
mivi_status_t mivi_estimate_gradient(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx,
                                     void *value_dev, void *grad_dev);
/* Same, host buffers, synchronous; additionally returns MIVI_ERR_NONFINITE when !isfinite(value)
 * (the check `step` performs at src/algorithms/common.jl:83-89). */
mivi_status_t mivi_estimate_gradient_host(mivi_ctx_t *ctx, const void *params_host, uint64_t estimate_idx,
                                          void *value_host, void *grad_host);
/* `count` consecutive estimates estimate_idx0 .. estimate_idx0+count-1 of the same params replayed as ONE
 * hipGraph launch; value/grad hold the LAST estimate on return.  Built-in targets only.  Mean-field family with the
 * diagonal-Gaussian target (rows independent): all `count` estimates run inside one launch-free kernel instead.  Full-rank f32 family,
 * d and n_mc multiples of 32 in [128, 2048] (multiples of 128 with the dense target or a sticking-the-landing estimator), Gaussian target:
 * the batch engine (kernels_fullrank_batch.hip) -- steps of up to 80 estimates as three launches (draws, one product, one VJP over all of
 * them), no graph. */
mivi_status_t mivi_estimate_gradient_n(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx0,
                                       int32_t count, void *value_dev, void *grad_dev);
/* The same batch with EVERY estimate's result kept: values_dev T[count] <- -elbo of estimate estimate_idx0 + i;
 * grads_dev T[count * params_len] <- its gradient (row i), or NULL when only the values are wanted.  What a caller of
 * estimate_objective / estimate_gradient! at fixed parameters wants from many estimates -- monitoring with many samples
 * (test/algorithms/klminrepgraddescent.jl:36), a gradient averaged over several estimates
 * (src/algorithms/repgradelbo.jl:151-177 called `count` times on one q).  Estimate i equals mivi_estimate_gradient(estimate_idx0 + i): bitwise on the generic route, to
 * rounding (value 1e-6, gradient relative l2 2e-6) on the batch engine (full-rank f32, d and n_mc multiples of 32, Gaussian targets). */
mivi_status_t mivi_estimate_gradient_each(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx0,
                                          int32_t count, void *values_dev, void *grads_dev);

/* estimate_gradient!(rng, obj::ScoreGradELBO, adtype, out, state, params, restructure): src/algorithms/scoregradelbo.jl:96-117
 * with AD of estimate_scoregradelbo_ad_forward (:87-94) replaced by its closed form (DESIGN.md "Score-gradient estimator").
 * With f_m = log q(z_m) - log pi(z_m) over the cfg.n_mc samples of `estimate_idx` -- the draws mivi_sample returns for that index:
 *   value_dev T[1] <- mean((f - mean f)^2) / 2   (the VarGrad objective, biased variance as :93)
 *   elbo_dev  T[1] <- mean(log pi - log q)       (the `stat` of :113-115; may be NULL)
 *   grad_dev  T[params_len] <- the gradient through log q alone, fully overwritten (full-rank: exact zeros above the diagonal)
 * Only VALUES of the target are used: every built-in target, the gradient callback (fn_value when set, otherwise the values fn_grad
 * returns) and the value-only callback, with or without a Stacked bijector (log pi gains logabsdetjac).  cfg.entropy is ignored.
 * n_mc = 1 gives value = 0 and a zero gradient exactly.  Asynchronous for built-in targets, synchronous for callback targets; a
 * non-finite value / elbo or a non-positive scale diagonal sets the sticky device flag like mivi_estimate_gradient.
 * MIVI_ERR_UNSUPPORTED: a sharded context (m_offset != 0 or m_total not in {0, n_mc}: the centring needs every sample); a full-rank d
 * beyond the LDS-resident triangular solve (the limit of the sticking-the-landing estimators). */
mivi_status_t mivi_estimate_score_gradient(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx,
                                           void *value_dev, void *elbo_dev, void *grad_dev);
/* Same, host buffers, synchronous; returns MIVI_ERR_NONFINITE / MIVI_ERR_NONPOSITIVE_SCALE (src/algorithms/common.jl:83-89). */
mivi_status_t mivi_estimate_score_gradient_host(mivi_ctx_t *ctx, const void *params_host, uint64_t estimate_idx,
                                                void *value_host, void *elbo_host, void *grad_host);

/* estimate_objective(rng, obj::RepGradELBO, q, prob; n_samples): src/algorithms/repgradelbo.jl:112-118;
 * `entropy` override mirrors the algorithm-level wrapper src/algorithms/common.jl:29-38 (default there:
 * MonteCarloEntropy).  n_samples may differ from cfg.n_mc: sample m of the call is column m of estimate_idx's eps stream whatever route
 * runs it (chunks of 16384 samples; on batch-engine configurations whole blocks of n_mc samples as engine lanes).  value_dev: T[1]. */
mivi_status_t mivi_estimate_objective(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx,
                                      int32_t n_samples, int32_t entropy, void *value_dev);
mivi_status_t mivi_estimate_objective_host(mivi_ctx_t *ctx, const void *params_host, uint64_t estimate_idx,
                                           int32_t n_samples, int32_t entropy, void *value_host);

/* gaussian_expectation_gradient_and_hessian!(rng, q, n_samples, grad_buf, hess_buf, prob), the first-order
 * (Stein / Price identity) branch: src/algorithms/gauss_expected_grad_hess.jl:20-60 -- the inner estimator of
 * KLMinWassFwdBwd / KLMinNaturalGradDescent / KLMinSqrtNaturalGradDescent (klminwassfwdbwd.jl:101,
 * klminnaturalgraddescent.jl:120, klminsqrtnaturalgraddescent.jl:104).  Full-rank family only (the reference method
 * takes a triangular scale).  With u = the eps stream of `estimate_idx` (d x n_samples) and z = C u + m:
 *   logpi_avg_dev T[1]    <- mean_b logpi(z_b)
 *   grad_dev      T[d]    <- mean_b grad logpi(z_b)
 *   hess_dev      T[d*d]  <- C' \ mean_b(u_b grad logpi(z_b)')      column-major, NOT symmetrised (as the reference)
 * n_samples <= 0 means cfg.n_mc; any n_samples is processed in chunks of 16384 columns.  Asynchronous for built-in
 * targets.  The second-order branch is mivi_gauss_expected_grad_hess2 below. */
mivi_status_t mivi_gauss_expected_grad_hess(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx,
                                            int32_t n_samples, void *logpi_avg_dev, void *grad_dev, void *hess_dev);
mivi_status_t mivi_gauss_expected_grad_hess_host(mivi_ctx_t *ctx, const void *params_host, uint64_t estimate_idx,
                                                 int32_t n_samples, void *logpi_avg_host, void *grad_host, void *hess_host);

/* The second-order branch of the same function (src/algorithms/gauss_expected_grad_hess.jl:61-83; the reference's test runs both
 * capabilities, test/general/gauss_expected_grad_hess.jl:45-56): for a target with second-order capability
 * (LogDensityProblems.logdensity_gradient_and_hessian) the Hessian estimate is the SAMPLE AVERAGE of the Hessians at z_b = C u_b + m
 * (the same eps stream as the first-order branch), no Stein identity and no solve:
 *   logpi_avg <- mean_b logpi(z_b)     grad <- mean_b grad logpi(z_b)     hess <- mean_b hess logpi(z_b)   (d x d column-major)
 * Targets with a Hessian: the built-in diagonal / dense Gaussians (constant Hessians -1/sigma^2 / -P: written exactly); the built-in
 * logistic regression (both variants, also on a row selection) and the funnel (unconstrained and constrained) -- their Hessians are linear
 * in per-sample statistics, so the average is one weighted Gram matrix X' diag(mean_b pi (1 - pi)) X resp. an arrow matrix, f64 sums
 * (csrc/kernels_hess2.hip); or a plugin that registered a batched Hessian callback next to its order-1 callback -- Z (d x M) in; ell (M),
 * G (d x M) and Hsum (d x d, column-major) = the SUM over the M columns of hess logpi(z_m) out, host buffers, non-zero return aborts.
 * A Stacked bijector around the target: MIVI_ERR_UNSUPPORTED (use the first-order entry, as the reference does for order-1 problems). */
typedef int32_t (*mivi_logdensity_gradient_and_hessian_fn)(void *user, const void *Z_host, int32_t d, int32_t M,
                                                           void *ell_host, void *G_host, void *Hsum_host);
mivi_status_t mivi_set_target_hess_callback(mivi_ctx_t *ctx, mivi_logdensity_gradient_and_hessian_fn fn, void *user);
mivi_status_t mivi_gauss_expected_grad_hess2(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx,
                                             int32_t n_samples, void *logpi_avg_dev, void *grad_dev, void *hess_dev);
mivi_status_t mivi_gauss_expected_grad_hess2_host(mivi_ctx_t *ctx, const void *params_host, uint64_t estimate_idx,
                                                  int32_t n_samples, void *logpi_avg_host, void *grad_host, void *hess_host);

/* KLMinSqrtNaturalGradDescent: the update of `step` (src/algorithms/klminsqrtnaturalgraddescent.jl:108-112) on the device-resident
 * parameters [m; vec(C)] of a full-rank context, IN PLACE, from grad (T[d]) and hess (T[d*d], column-major) as the estimator entries above
 * leave them -- both read-only, hess used as it comes (not symmetrised, not transposed; only the lower triangle of A is formed):
 *   A = C' (-hess) C - I     T = tril(A) - diag(A)/2     m' = m - stepsize C (C' (-grad))     C' = C - stepsize C T   (exact zeros above the diagonal)
 *   entropy_dev T[1] <- entropy(q') = d/2 (1 + log 2 pi) + sum_i log C'_ii  (src/families/location_scale.jl:52-57; the term of :119); may be NULL
 * d <= 48: one workgroup, one launch; above: three launches of 64 x 64 tiles on the matrix cores (csrc/kernels_ngd.hip), C' assembled from a
 * context-owned copy of C.  The update is bitwise repeatable (no floating-point atomics, one summation order).  A C'_ii that is not a positive finite number or a non-finite entropy sets the sticky device flag
 * (mivi_synchronize); the _host form (host buffers, synchronous) returns MIVI_ERR_NONPOSITIVE_SCALE / MIVI_ERR_NONFINITE itself.  Any d >= 1.
 * MIVI_ERR_UNSUPPORTED: a mean-field context. */
mivi_status_t mivi_sqrt_ngd_update(mivi_ctx_t *ctx, void *params_dev, const void *grad_dev, const void *hess_dev, double stepsize,
                                   void *entropy_dev);
mivi_status_t mivi_sqrt_ngd_update_host(mivi_ctx_t *ctx, void *params_host, const void *grad_host, const void *hess_host, double stepsize,
                                        void *entropy_host);
/* `count` whole iterations of step(rng, alg::KLMinSqrtNaturalGradDescent, ...) (src/algorithms/klminsqrtnaturalgraddescent.jl:79-127, without
 * subsampling and callback) with the parameters resident in HBM and no host round trip: iteration t estimates with index estimate_idx0 + t
 * (:104; second_order = 0: mivi_gauss_expected_grad_hess, the Stein branch; != 0: mivi_gauss_expected_grad_hess2; n_samples <= 0: cfg.n_mc), then
 * updates (:108-112); elbo_dev T[count] (or NULL) <- logpi_avg_t + entropy(q'_t) (:119).  The same launches and arithmetic as `count` calls of the estimator entry followed by
 * mivi_sqrt_ngd_update: bitwise equal to them and bitwise repeatable wherever the estimator entry is (the second-order branch of the built-in logistic-regression and
 * funnel targets sums with f64 atomics, csrc/kernels_hess2.hip: those steps repeat to the rounding of a reordered f64 sum).  Asynchronous for built-in targets, synchronous per step for callback targets; a non-finite elbo or a C'_ii that is
 * not positive sets the sticky device flag.  MIVI_ERR_UNSUPPORTED: a mean-field context (:58 takes a LowerTriangular scale); a sharded context; what
 * the chosen estimator entry refuses (second_order without a Hessian or under a Stacked bijector; d beyond the first-order entry's solve). */
mivi_status_t mivi_sqrt_ngd_steps(mivi_ctx_t *ctx, void *params_dev, uint64_t estimate_idx0, int32_t count, int32_t n_samples,
                                  int32_t second_order, double stepsize, void *elbo_dev);

/* KLMinNaturalGradDescent (variational online Newton, src/algorithms/klminnaturalgraddescent.jl).  Besides the parameters [m; vec(C)] the
 * algorithm carries state_dev T[2*d*d] = [S; Sigma]: the precision (`prec`) and the covariance (`qcov`) of q, d x d column-major, both stored
 * as full symmetric matrices with the two triangles bitwise mirrored, carried from step to step and not recomputed from the scale.
 * mivi_natgrad_init (:83-87): S <- C^-T C^-1 (a triangular inverse and one product), Sigma <- C C'; params_dev is only read.
 * mivi_natgrad_update (:129-145), params and state IN PLACE, grad (T[d]) and hess (T[d*d], column-major) read-only and hess used as it comes:
 *   ensure_posdef != 0:  Gh = S + hess    S' = Hermitian(S - eta Gh + eta^2/2 Gh Sigma Gh)   (:129-130)
 *   ensure_posdef == 0:                   S' = Hermitian((1 - eta) S - eta hess)             (:132)
 *   S' = Lr' Lr (Lr lower triangular)     C' = Lr^-1     Sigma' = C' C''     m' = m - eta C' (C'' (-grad))   (:134-139)
 *   entropy_dev T[1] <- entropy(q') = d/2 (1 + log 2 pi) + sum_i log C'_ii (the term of :145); may be NULL
 * Hermitian(.) is the reference's: the UPPER triangle of the operand, mirrored (not the symmetric part; hess is not symmetric on the Stein
 * branch).  SCALE CONVENTION, the one deviation from the reference: its new scale is the upper-triangular adjoint of the inverse of a lower
 * Cholesky factor of S' (:136-138); this library's full-rank family stores a lower-triangular C with exact zeros above the diagonal, so the
 * iterate is q' = (m', C') with C' the LOWER Cholesky factor of Sigma' = S'^-1 -- the same distribution and the same recursion in
 * (m, S, Sigma) as a function of (grad, hess); only the pairing of draws with samples differs (z = C' u + m).
 * d <= MIVI_NATGRAD_SMALL_D: one workgroup, one launch; above: 64 x 64 tiles on the matrix cores over context-owned padded scratch, a blocked
 * factorisation by 64-row panels and a blocked triangular inverse (csrc/kernels_natgrad.hip; 3 nT + 5 launches, + 2 with ensure_posdef,
 * nT = ceil(d / 64)).  m' is formed as m - eta x with x = C' C'' (-grad) refined once against S' (r = -grad - S' x, x += C' C'' r; float64
 * sums), which an ill-conditioned S' needs in float32.  Bitwise repeatable (no floating-point atomics, one summation order).  A pivot that is not a positive finite number
 * (the reference throws PosDefException there) or a non-finite entropy sets the sticky device flag (mivi_synchronize:
 * MIVI_ERR_NONPOSITIVE_SCALE / MIVI_ERR_NONFINITE); the pivot is replaced by 1, the call returns, and the contents of params and state are
 * then unspecified.  The _host form (host buffers, synchronous) returns the status itself.  Any d >= 1.  MIVI_ERR_UNSUPPORTED: a mean-field context. */
#define MIVI_NATGRAD_SMALL_D 44
mivi_status_t mivi_natgrad_init(mivi_ctx_t *ctx, const void *params_dev, void *state_dev);
mivi_status_t mivi_natgrad_update(mivi_ctx_t *ctx, void *params_dev, void *state_dev, const void *grad_dev, const void *hess_dev,
                                  double stepsize, int32_t ensure_posdef, void *entropy_dev);
mivi_status_t mivi_natgrad_update_host(mivi_ctx_t *ctx, void *params_host, void *state_host, const void *grad_host, const void *hess_host,
                                       double stepsize, int32_t ensure_posdef, void *entropy_host);
/* `count` whole iterations of step(rng, alg::KLMinNaturalGradDescent, ...) (src/algorithms/klminnaturalgraddescent.jl:95-153, without
 * subsampling and callback), parameters and state resident in HBM and no host round trip: iteration t estimates with index estimate_idx0 + t
 * (:120; second_order as for mivi_sqrt_ngd_steps), then updates; elbo_dev T[count] (or NULL) <- logpi_avg_t + entropy(q'_t) (:145), written
 * with the flags by the update's last launch.  The same launches and arithmetic as `count` calls of the estimator entry followed by
 * mivi_natgrad_update: bitwise equal to them.  Asynchronous for built-in targets.  Refusals as for mivi_sqrt_ngd_steps (a mean-field
 * context, a sharded context, no target, what the chosen estimator entry refuses); a refused call launches nothing.  Like the reference it
 * does not require ensure_posdef for the first-order branch. */
mivi_status_t mivi_natgrad_steps(mivi_ctx_t *ctx, void *params_dev, void *state_dev, uint64_t estimate_idx0, int32_t count, int32_t n_samples,
                                 int32_t second_order, double stepsize, int32_t ensure_posdef, void *elbo_dev);

/* FisherMinBatchMatch ("batch and match", src/algorithms/fisherminbatchmatch.jl): the covariance-weighted Fisher divergence minimiser.  It
 * needs gradients only and takes no step size.  Besides [m; vec(C)] it carries state_dev T[d*d] = Sigma, the covariance (`sigma`, :49), d x d
 * column-major, a full symmetric matrix with bitwise-mirrored triangles, carried from step to step.  With u (d x B) standard normal,
 * z = C u + m, g_b = grad logpi(z_b) and lambda = d B / iteration:
 *   mivi_bam_init (:76): state_dev <- C C'; params_dev is only read.
 *   mivi_bam_moments (rand_batch_match_samples_with_objective!, :81-111, and the elbo of :157): u_dev, G_dev T[d*n_samples] column-major <- the
 *     draws (bitwise the eps mivi_sample returns for estimate_idx on a context with n_mc = n_samples) and the per-sample gradients;
 *     fisher_dev <- sum |u + C' G|^2 / n_samples (:108); logpi_avg_dev <- mean_b logpi(z_b) (:99); elbo_dev <- logpi_avg + entropy(q) (:157).
 *     2 <= n_samples <= 16384.  Asynchronous for built-in targets, synchronous for callback targets.  The same eps stream and sample / target
 *     kernels as mivi_gauss_expected_grad_hess.
 *   mivi_estimate_fisher (estimate_objective, :186-195): value_dev <- the same fisher for ANY n_samples >= 2, in chunks of 16384 columns.
 *   mivi_bam_update (:143-155): (m, C, Sigma) -> (m', C', Sigma') IN PLACE from u_dev and G_dev (read-only), n_samples = B columns:
 *       zbar, Cz = mean_and_cov(z)   gbar, Gamma = mean_and_cov(G)   (corrected, 1/(B-1))
 *       U = lambda Gamma + lambda/(1+lambda) gbar gbar'      V = Sigma + lambda Cz + lambda/(1+lambda) (m - zbar)(m - zbar)'
 *       Sigma' = 2 V (I + sqrt(I + 4 U V))^-1     m' = m/(1+lambda) + lambda/(1+lambda) (Sigma' gbar + zbar)     C' = cholesky(Sigma').L
 *     entropy_dev T[1] <- entropy(q') (may be NULL).  C' is lower triangular with exact zeros above the diagonal: the reference's own scale,
 *     no deviation.  The matrix square root of the non-symmetric U V is taken through the rank-B form of the batch-and-match paper
 *     (csrc/kernels_bam.hip): one B x B symmetric eigenproblem (cyclic Jacobi in one workgroup, a compile-time bound on
 *     its sweeps), thin products on the matrix cores and ONE blocked factorisation (that of mivi_natgrad_update); float64 arithmetic for
 *     either context type; 2 nT + 6 launches, nT = ceil(d / 64).  Bitwise repeatable.  A pivot that is not a positive finite number sets the
 *     sticky flag of MIVI_ERR_NONPOSITIVE_SCALE and is replaced by 1; an eigenproblem that does not converge within the bound (a NaN in G)
 *     or a non-finite entropy sets that of MIVI_ERR_NONFINITE; the call returns and the contents of params and state are then unspecified.
 *     lambda > 0 is the caller's d B / iteration, converted to the parameters' element type as the reference does (:148).
 *   mivi_bam_steps (step, :113-167, without subsampling and callback): `count` whole steps with no host round trip; step t estimates with
 *     index estimate_idx0 + t and uses lambda = d n_samples / (iteration0 + t) (iteration0 >= 1); fisher_dev, elbo_dev T[count] (or NULL) <-
 *     the objective and elbo at the iterate each step STARTS from (:157-158).  The same launches and arithmetic as mivi_bam_moments
 *     followed by mivi_bam_update: bitwise equal to them.
 * The _host forms take host buffers, are synchronous and return the sticky status themselves.
 * Every entry refuses, before anything launches and leaving params and state untouched: a mean-field context, a sharded context, a Stacked
 * bijector (MIVI_ERR_UNSUPPORTED: the algorithm requires unconstrained support); no target (MIVI_ERR_NO_TARGET); n_samples < 2
 * (MIVI_ERR_BAD_ARG: the corrected covariance is undefined); n_samples > MIVI_BAM_MAX_SAMPLES for the update and the steps entry
 * (MIVI_ERR_UNSUPPORTED: more needs a multi-workgroup eigen-solver). */
#define MIVI_BAM_MAX_SAMPLES 64
mivi_status_t mivi_bam_init(mivi_ctx_t *ctx, const void *params_dev, void *state_dev);
mivi_status_t mivi_bam_moments(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx, int32_t n_samples, void *u_dev, void *G_dev,
                               void *fisher_dev, void *logpi_avg_dev, void *elbo_dev);
mivi_status_t mivi_bam_moments_host(mivi_ctx_t *ctx, const void *params_host, uint64_t estimate_idx, int32_t n_samples, void *u_host, void *G_host,
                                    void *fisher_host, void *logpi_avg_host, void *elbo_host);
mivi_status_t mivi_estimate_fisher(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx, int32_t n_samples, void *value_dev);
mivi_status_t mivi_estimate_fisher_host(mivi_ctx_t *ctx, const void *params_host, uint64_t estimate_idx, int32_t n_samples, void *value_host);
mivi_status_t mivi_bam_update(mivi_ctx_t *ctx, void *params_dev, void *state_dev, const void *u_dev, const void *G_dev, int32_t n_samples,
                              double lambda, void *entropy_dev);
mivi_status_t mivi_bam_update_host(mivi_ctx_t *ctx, void *params_host, void *state_host, const void *u_host, const void *G_host,
                                   int32_t n_samples, double lambda, void *entropy_host);
mivi_status_t mivi_bam_steps(mivi_ctx_t *ctx, void *params_dev, void *state_dev, uint64_t estimate_idx0, uint64_t iteration0, int32_t count,
                             int32_t n_samples, void *fisher_dev, void *elbo_dev);

/* KLMinWassFwdBwd (stochastic proximal gradient descent in Wasserstein space, src/algorithms/klminwassfwdbwd.jl).  Besides [m; vec(C)] it
 * carries state_dev T[d*d] = Sigma, the covariance (`sigma`, :49), d x d column-major, a full symmetric matrix with bitwise-mirrored
 * triangles, carried from step to step.
 *   mivi_wass_init (:75): state_dev <- C C' (the launch of mivi_bam_init); params_dev is only read.
 *   mivi_wass_update (:105-114), params and state IN PLACE, grad (T[d]) and hess (T[d*d], column-major) read-only and hess used as it comes
 *   (not symmetric on the Stein branch; note the transpose), eta = stepsize converted to T (:88):
 *       m' = m + eta grad        M = I + eta hess'        Sh = Hermitian(M Sigma M')                                     (:105-107)
 *       Sigma' = (Sh + 2 eta I + sqrt(Hermitian(Sh (Sh + 4 eta I)))) / 2        C' = cholesky(Sigma').L                   (:110-111)
 *       entropy_dev T[1] <- entropy(q') = d/2 (1 + log 2 pi) + sum_i log C'_ii (the term of :114); may be NULL
 *     Hermitian(.) is the reference's: the UPPER triangle of the operand, mirrored.  C' is lower triangular with exact zeros above the
 *     diagonal: the reference's own scale, no deviation.  The symmetric square root is not an eigendecomposition but the coupled
 *     Newton-Schulz iteration on the matrix cores (csrc/kernels_wass.hip): A = Hermitian(Sh (Sh + 4 eta I)),
 *     c = |A|_F, Y_0 = A / c, Z_0 = I, E_k = I - Z_k Y_k, Y_k+1 = Y_k + Y_k E_k / 2, Z_k+1 = Z_k + E_k Z_k / 2, sqrt(A) = sqrt(c) (Y + Y')/2,
 *     stopped on the device at the first round with |E_k|_F <= 64 d eps or, from the fifth round on, with |E_k|_F no longer halving below
 *     1e-6 or growing; at most MIVI_WASS_MAX_ROUNDS rounds.  Float64 arithmetic for either context type.
 *     2 nT + 2 MIVI_WASS_MAX_ROUNDS + 5 launches, nT = ceil(d / 64) (the rounds after the stop return at once), the last 2 nT of them the
 *     blocked factorisation of mivi_natgrad_update and its finish.  Bitwise repeatable (no floating-point atomics, one summation order).
 *     A pivot that is not a positive finite number sets the sticky flag of MIVI_ERR_NONPOSITIVE_SCALE and is replaced by 1; an iteration
 *     that does not stop within the bound, a non-finite |E_k|_F (a NaN in grad or hess) or a non-finite entropy sets that of
 *     MIVI_ERR_NONFINITE; the call returns and the contents of params and state are then unspecified.  The _host form (host buffers,
 *     synchronous) returns the status itself.  Any d >= 1.  MIVI_ERR_UNSUPPORTED: a mean-field context.
 *   mivi_wass_steps (step, :80-122, without subsampling and callback): `count` whole iterations with no host round trip: iteration t
 *     estimates with index estimate_idx0 + t (:101; second_order as for mivi_sqrt_ngd_steps), then updates; elbo_dev T[count] (or NULL) <-
 *     logpi_avg_t + entropy(q'_t) (:114).  The same launches and arithmetic as `count` calls of the estimator entry followed by
 *     mivi_wass_update: bitwise equal to them.  Refusals as for mivi_natgrad_steps (a mean-field context, a sharded context, no target, what
 *     the chosen estimator entry refuses); a refused call launches nothing. */
#define MIVI_WASS_MAX_ROUNDS 64
mivi_status_t mivi_wass_init(mivi_ctx_t *ctx, const void *params_dev, void *state_dev);
mivi_status_t mivi_wass_update(mivi_ctx_t *ctx, void *params_dev, void *state_dev, const void *grad_dev, const void *hess_dev, double stepsize,
                               void *entropy_dev);
mivi_status_t mivi_wass_update_host(mivi_ctx_t *ctx, void *params_host, void *state_host, const void *grad_host, const void *hess_host,
                                    double stepsize, void *entropy_host);
mivi_status_t mivi_wass_steps(mivi_ctx_t *ctx, void *params_dev, void *state_dev, uint64_t estimate_idx0, int32_t count, int32_t n_samples,
                              int32_t second_order, double stepsize, void *elbo_dev);

/* ---- multi-GPU: shard the MC batch, all-reduce the partials, finalize -------------------------- *
 * No counterpart in the reference (single task).  partials_dev: T[partials_len] un-normalised sums over
 * this context's samples; the caller all-reduces (RCCL sum) and calls mivi_finalize on every rank. */
mivi_status_t mivi_estimate_partials(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx,
                                     void *partials_dev);
mivi_status_t mivi_finalize(mivi_ctx_t *ctx, const void *params_dev, const void *partials_dev,
                            void *value_dev, void *grad_dev);

/* ---- next to the hot path: projection + optimiser step, device-resident ---------- */
/* ClipScale: scale[diagind] = max(scale[diagind], eps)   src/optimization/clip_scale.jl:18-29; low-rank family: scale_diag, params[d .. 2d)
 * (clip_scale.jl:31-41) */
mivi_status_t mivi_clip_scale(mivi_ctx_t *ctx, void *params_dev, double epsilon);
/* Optimisers.Descent(eta): params .-= eta .* grad  (the rule of test/algorithms/klminrepgraddescent.jl:110) */
mivi_status_t mivi_descent_update(mivi_ctx_t *ctx, void *params_dev, const void *grad_dev, double eta);
/* Optimisers.Adam(eta, (b1,b2), eps) (bench/benchmarks.jl:64): state_dev T[2*params_len] (m; v), t = step number >= 1 */
mivi_status_t mivi_adam_update(mivi_ctx_t *ctx, void *params_dev, const void *grad_dev, void *state_dev,
                               int64_t t, double eta, double beta1, double beta2, double eps);
/* COCOB(alpha), the "COCOB-Backprop" coin-betting rule (src/optimization/rules.jl:78-96): state_dev T[5*params_len] =
 * (L; G; R; theta; x1), initialised by the caller to (0; 0; 0; 0; params) as Optimisers.init does (:84-86).  Coordinates whose
 * gradient has been exactly zero so far (L = 0; the reference's expression is 0/0 there) are left unchanged. */
mivi_status_t mivi_cocob_update(mivi_ctx_t *ctx, void *params_dev, const void *grad_dev, void *state_dev, double alpha);
/* y <- a*x + b*y over n elements of T.  PolynomialAveraging: x_bar = (1-w) x_bar + w x, src/optimization/averaging.jl:40-47 */
mivi_status_t mivi_axpby(mivi_ctx_t *ctx, void *y_dev, double a, const void *x_dev, double b, int64_t n);
/* DoG (kind 0) / DoWG (kind 1): src/optimization/rules.jl:48-64 / :17-34.  state_dev holds x0 (T[params_len]) followed
 * by two doubles (v, r) at byte offset mivi_dog_state_bytes(ctx)-16.  init: x0 = params, v = 0, r = alpha*(1+norm(params)). */
int64_t mivi_dog_state_bytes(const mivi_ctx_t *ctx);
mivi_status_t mivi_dog_init(mivi_ctx_t *ctx, const void *params_dev, void *state_dev, double alpha);
mivi_status_t mivi_dog_update(mivi_ctx_t *ctx, void *params_dev, const void *grad_dev, void *state_dev, int32_t kind);
/* ProximalLocationScaleEntropy (src/optimization/proximal_location_scale_entropy.jl:44-61), the operator of
 * KLMinRepGradProxDescent (src/algorithms/constructors.jl:122-157): every scale-diagonal entry
 * c <- c + (sqrt(c^2 + 4 gamma) - c) / 2.  gamma = `stepsize` (Descent: eta) when dog_state_dev is NULL, otherwise it is read
 * on the device from the DoG / DoWG state (r / sqrt(v) resp. r^2 / sqrt(v), :26-42) -- no host round trip. */
mivi_status_t mivi_prox_scale_entropy(mivi_ctx_t *ctx, void *params_dev, double stepsize, const void *dog_state_dev,
                                      int32_t dog_kind);
/* `n_steps` iterations of src/algorithms/common.jl:69-104 {estimate_gradient!, update!, ClipScale} with params
 * resident in HBM; rule: 0 = Descent(eta), 1 = Adam(eta).  elbo_dev: T[n_steps] or NULL receives info.elbo (= -value) per
 * iteration.  Returns MIVI_ERR_NONFINITE if any objective was not finite.
 * What runs (first match; every launch-free form keeps parameters and optimiser state in registers for all n_steps):
 *   mean-field, diagonal-Gaussian target                      one launch-free kernel (rows are independent), bitwise the single calls
 *                                                             (sticking-the-landing estimators: a few entries one ulp apart -- the two
 *                                                             kernels' residual terms are contracted differently by the compiler)
 *   full-rank, d <= 32, d n_mc <= 768 (STL 512)              one workgroup for the whole loop (the reference's own benchmark grid), to rounding
 *   full-rank f32, n_mc <= 32, diagonal-Gaussian target,      row-separable launch-free kernel (workgroups own row pairs), to rounding
 *     closed-form / Monte-Carlo entropy, d <= 1126
 *   mean-field, fused funnel target                           one kernel with a per-step grid-wide exchange, bitwise the single calls
 *   logistic-regression target, (d - 1) n_mc <= 256, d <= 64,  one kernel for the whole loop (the reference README's own example: one workgroup;
 *     n (d - 1) n_mc <= 2^20                                  larger data sets: up to 64 that split the rows and exchange partial sums), to rounding
 *   otherwise                                                 one hipGraph of chained estimates (full-rank f32: update + ClipScale in the VJP epilogue)
 *   K independent runs of the one-workgroup shapes above       mivi_optimize_loop_many: the same two kernels, workgroup k = run k (below)
 * MIVI_NO_FUSED_LOOP=1 forces the hipGraph everywhere (A/B). */
mivi_status_t mivi_optimize_steps(mivi_ctx_t *ctx, void *params_dev, void *opt_state_dev, uint64_t estimate_idx0,
                                  int64_t t0, int32_t n_steps, int32_t rule, double eta, double clip_epsilon,
                                  void *elbo_dev);

/* The general device-resident loop: `n_steps` iterations of `step` (src/algorithms/common.jl:69-104)
 *     estimate_gradient!  ->  Optimisers.update!  ->  operator  ->  averager
 * for every rule / operator / averager the reference's ParamSpaceSGD algorithms combine (constructors.jl:44-157):
 *   rule      0 Descent(eta) | 1 Adam(eta, beta1, beta2, adam_eps) | 2 DoG | 3 DoWG      (src/optimization/rules.jl:17-64)
 *             4 COCOB(alpha = eta)                                                         (src/optimization/rules.jl:66-96)
 *   op        0 IdentityOperator | 1 ClipScale(clip_epsilon) | 2 ProximalLocationScaleEntropy (step size from the rule)
 *   averager  0 NoAveraging | 1 PolynomialAveraging(avg_eta): x_bar <- (1-w_t) x_bar + w_t x, w_t = (eta+1)/(t+eta)
 * opt_state: Adam T[2 params_len] (zeros before the first step) | DoG/DoWG mivi_dog_state_bytes (after mivi_dog_init) |
 * COCOB T[5 params_len] = [L; G; R; theta; x1] (zeros, x1 = the initial parameters: rules.jl:84-86).  COCOB runs as the hipGraph of chained
 * estimates with its update kernel (ClipScale fused), not in the launch-free loops; ProximalLocationScaleEntropy has no step size for it.
 * avg_params: T[params_len] running average, in/out (any content when t0 = 0: w_1 = 1).  t0 = iterations already done
 * (warm start, src/optimize.jl:58-62).  Descent/Adam with Identity/ClipScale and no averaging take the fused paths of
 * mivi_optimize_steps; the other combinations are launch-free as well where mivi_optimize_steps is (mean-field + diagonal-Gaussian
 * target, d <= 4096 (f64: 2048) for DoG / DoWG; full-rank with n_mc <= 32 or d <= 32 and that target), with DoG / DoWG exchanging two norm
 * partials per workgroup and step.  Results are bitwise those of the step-by-step entries on the hipGraph route and for
 * Descent / Adam on the mean-field loop; DoG / DoWG in the launch-free loops to the rounding of the two f64 norm sums, the
 * full-rank launch-free loops to f32 rounding. */
typedef struct mivi_loop {
  int32_t rule, op, averager, n_steps;
  double eta, beta1, beta2, adam_eps;
  double clip_epsilon, avg_eta;
  void *opt_state_dev;
  void *avg_params_dev;
  uint64_t estimate_idx0;
  int64_t t0;
  void *elbo_dev;     /* T[n_steps] or NULL: info.elbo of every iteration */
} mivi_loop_t;
mivi_status_t mivi_optimize_loop(mivi_ctx_t *ctx, void *params_dev, const mivi_loop_t *loop);
/* K INDEPENDENT runs of mivi_optimize_loop in ONE launch, workgroup k = run k: `optimize` (src/optimize.jl:42-94) called K times -- restarts
 * from other seeds and initialisations, a step-size sweep, one fit per simulated data set or bootstrap replicate -- for the small problems
 * whose whole loop of `step`s (src/algorithms/common.jl:69-104) fits one workgroup, the sizes of the reference's own benchmark
 * (bench/benchmarks.jl:43-94).  A single such run keeps one compute unit busy; K of them fill the device.  Two classes are served:
 *   A  full-rank family, diagonal-Gaussian target, d <= 32, n_mc <= 64, d n_mc <= 768 (512 with the sticking-the-landing estimators); every
 *      entropy estimator.  Per run: seed, first estimate index, eta, parameters, optimiser state, average, and the target's mean / std.
 *   B  logistic-regression target, both families, both variants, (d - 1) n_mc <= 256, d <= 64, n (d - 1) n_mc <= 2^20, and the run's y fits
 *      the LDS of ONE workgroup beside the kernel's other arrays (every run is one workgroup whatever mivi_optimize_loop would split; X is
 *      resident in LDS where it fits and streamed otherwise).  Per run: as A without the target, plus y and optionally X; n, p, variant and
 *      likeadj are the context's.
 * Rules 0-3, operators 0-2, averager 0 / 1, f32 and f64.  Every array is run-major: params_dev T[K params_len]; loop->opt_state_dev K times
 * the single run's state (Adam: 2 params_len elements, DoG / DoWG: mivi_dog_state_bytes bytes); loop->avg_params_dev T[K params_len];
 * loop->elbo_dev T[K n_steps].  loop->eta, estimate_idx0 hold for every run whose array below is NULL; t0, the betas, clip_epsilon and avg_eta
 * are common.  Run k executes the instructions of the single-run kernel on the same threads: mivi_optimize_loop on a context with run k's
 * seed and target gives the same bits where it is one workgroup too (always in class A; in class B where it does not split the rows), and
 * agrees to the rounding of the row sums elsewhere.  Workgroups never wait for one another, so K may exceed what is resident at once.
 * A run that diverges finishes its steps carrying NaNs and touches nothing of another run.
 *   n_runs               K >= 1
 *   seed_host            uint64[K] or NULL: the context's seed for every run
 *   estimate_idx0_host   uint64[K] or NULL: loop->estimate_idx0
 *   eta_host             double[K] or NULL: loop->eta
 *   mean_host, std_host  class A: T[K d] each (both or neither), or NULL: the context's target for every run
 *   y_dev                class B: device uint8[K n], or NULL: the context's y for every run
 *   X_dev, X_run_stride  class B: device X (n x p column-major) of run 0 and the elements between the runs' matrices (0: one matrix for all),
 *                        or NULL: the context's X.  Device data are borrowed for the call.
 *   status_host          int32[K] or NULL, written on return: bit 1 a non-finite objective, bit 2 a non-positive scale diagonal, per run
 * Returns MIVI_OK when the launch ran and status_host is given, whatever the per-run bits say; with status_host NULL a set bit in any run
 * returns what mivi_optimize_loop returns for it (MIVI_ERR_NONPOSITIVE_SCALE for bit 2, else MIVI_ERR_NONFINITE).  MIVI_ERR_UNSUPPORTED, with
 * a message naming the reason and before anything is uploaded: a configuration outside A / B, a Stacked bijector, a sharded context, a batch
 * schedule, an index source, the low-rank family, a non-normal base, rule 4 (COCOB), MIVI_NO_FUSED_LOOP=1.  MIVI_ERR_BAD_ARG: n_runs < 1, a
 * non-positive std, op = 2 with Adam, a target array of the other class.  The call waits for the runs (it reads their status words).
 * mivi_batch_info(what = 7) then reports 16 | the id of the loop whose kernel ran. */
typedef struct mivi_many {
  int32_t n_runs;
  const uint64_t *seed_host;
  const uint64_t *estimate_idx0_host;
  const double *eta_host;
  const void *mean_host;
  const void *std_host;
  const uint8_t *y_dev;
  const void *X_dev;
  int64_t X_run_stride;
  int32_t *status_host;
} mivi_many_t;
mivi_status_t mivi_optimize_loop_many(mivi_ctx_t *ctx, void *params_dev, const mivi_loop_t *loop, const mivi_many_t *many);
/* mivi_optimize_loop on a scheduled context (mivi_logreg_set_batch_schedule) where step t (0-based) evaluates batch first_batch + t: whole
 * steps of a SubsampledObjective (src/algorithms/subsampledobjective.jl:64-90) on the device.  When the schedule carries estimate indices,
 * step t draws at estimate_idx_host[first_batch + t] (loop->estimate_idx0 is not read), otherwise at estimate_idx0 + t.  Requires
 * 0 <= first_batch and first_batch + n_steps <= n_batches (MIVI_ERR_BAD_ARG).  Runs as the hipGraph of chained estimates -- a step's batch
 * is a kernel argument, its index a device word of the uploaded table -- recorded once per (loop configuration, first_batch); every rule,
 * operator and averager, elbo_dev, the sticky status and the non-finite behaviour of mivi_optimize_loop.  The selected batch is unchanged. */
mivi_status_t mivi_optimize_loop_batches(mivi_ctx_t *ctx, void *params_dev, const mivi_loop_t *loop, int32_t first_batch);

/* Estimate-index source: when idx_dev != NULL every estimate uses estimate_idx + *idx_dev (read on the device at
 * kernel time), so a captured graph (e.g. a torch CUDAGraph holding kernels + the RCCL all-reduce) advances the
 * eps stream on replay by bumping one device word.  NULL restores by-value indices. */
mivi_status_t mivi_set_index_source(mivi_ctx_t *ctx, const uint64_t *idx_dev);

/* Tools / tests: which kernels evaluate the built-in logistic regression (f32): 0 = by problem size (default: the VALU
 * kernels below n*p*n_mc = 1.6e7, the matrix-core kernels above), 1 = matrix-core kernels, 2 = VALU kernels.  Results
 * agree to rounding; f64 always takes the VALU kernels. */
mivi_status_t mivi_set_logreg_route(mivi_ctx_t *ctx, int32_t route);

/* ---- sharded finalisation + the collective behind the ABI --------------------------------------------------
 * The Monte-Carlo mean of src/algorithms/repgradelbo.jl:84-86 shards over the sample axis; what crosses GPUs is the partial
 * vector of mivi_estimate_partials.  Instead of all-reduce + a finalisation replicated on every rank:
 *     reduce-scatter  ->  every rank finalises ITS slice (mivi_finalize_slice)  ->  all-gather  ->  unpack (mivi_unpack_final)
 * The slice of rank r is elements [r * n, (r + 1) * n) of the partial vector padded to n * world, n = mivi_slice_len(ctx, world).
 * The packed "final" vector has the layout of the partial vector: [d/dmu; d/dsigma or the column-packed lower triangle of d/dC;
 * value; status bits].  Both functions are plain kernels on the context's stream: a host that owns its collectives
 * (torch.distributed, MPI.jl, RCCL from Julia) calls them around its own reduce-scatter / all-gather. */
int64_t mivi_slice_len(const mivi_ctx_t *ctx, int32_t world);
mivi_status_t mivi_finalize_slice(mivi_ctx_t *ctx, const void *params_dev, const void *slice_sum_dev, int32_t rank, int32_t world,
                                  void *final_slice_dev);
mivi_status_t mivi_unpack_final(mivi_ctx_t *ctx, const void *packed_final_dev, void *value_dev, void *grad_dev);

/* The collective itself, for hosts without one (julia/MIVI.jl): RCCL opened at run time (dlopen of librccl.so, override with
 * MIVI_RCCL_LIB; a copy the process already loaded is reused).  mivi_comm_unique_id fills 128 bytes on rank 0 (ship them to the
 * other ranks any way you like), mivi_comm_init joins `world` ranks -- one process per GPU, the context created with n_mc = the
 * local share, m_offset = its first global column, m_total = n_mc * world.  mivi_estimate_gradient_dist is then estimate_gradient!
 * of the m_total-sample estimate on every rank: {partials kernels, ncclReduceScatter, slice finalise, ncclAllGather, unpack}, all
 * on the context's stream (graph-capturable).  world = 1 without a communicator runs the same kernels without the collectives;
 * world = 1 WITH an id runs them through RCCL (single-GPU test of the whole path).  Route: see mivi_comm_set_route. */
#define MIVI_COMM_ID_BYTES 128
mivi_status_t mivi_comm_unique_id(void *id_host);
mivi_status_t mivi_comm_init(mivi_ctx_t *ctx, const void *id_host, int32_t rank, int32_t world);
mivi_status_t mivi_comm_destroy(mivi_ctx_t *ctx);
mivi_status_t mivi_estimate_gradient_dist(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx, void *value_dev, void *grad_dev);

/* The exchange written for xGMI (csrc/kernels_p2p.hip), no RCCL involved: every GPU of a node has a direct link to every other one, so
 * the sum of the partial vectors is ONE kernel per rank with two one-hop phases -- every rank stores slice s of its partial vector
 * straight into rank s's staging area; rank s sums the `world` contributions of its slice in rank order, finalises it (the owner of
 * the two scalars also assembles the objective value) and stores the packed final slice into every rank's final buffer; every rank
 * unpacks.  All ranks hold bit-identical results.  One fine-grained allocation per rank, mapped into its peers through HIP IPC:
 *   mivi_p2p_export   allocates this rank's exchange area and fills MIVI_P2P_HANDLE_BYTES describing it (world <= 8: one node);
 *   (the host gathers the `world` blobs in rank order by whatever channel it has: MPI, a file, torch.distributed, ...)
 *   mivi_p2p_attach   maps the peers' areas (ranks inside one process -- tests -- are mapped by pointer); the context then behaves as
 *                     rank `rank` of `world` for mivi_estimate_gradient_dist[_n] even without an RCCL communicator;
 *   mivi_comm_enable_p2p = export + gather through the RCCL communicator of mivi_comm_init + attach, for hosts with no other channel.
 * Every wait inside the kernel is bounded: a peer that never arrives makes the next mivi_synchronize return MIVI_ERR_HIP. */
#define MIVI_P2P_HANDLE_BYTES 256
mivi_status_t mivi_p2p_export(mivi_ctx_t *ctx, int32_t rank, int32_t world, void *handle_host);
mivi_status_t mivi_p2p_attach(mivi_ctx_t *ctx, const void *handles_host /* world x MIVI_P2P_HANDLE_BYTES, rank order */);
mivi_status_t mivi_p2p_detach(mivi_ctx_t *ctx);
/* host-only: out4 = {slice length n, chunk length cn, chunk workgroups G, rank that owns the two scalars} for a partial vector of
 * length L over `world` ranks (no GPU needed) */
void mivi_p2p_geometry(int64_t L, int32_t world, int64_t *out4);
mivi_status_t mivi_comm_enable_p2p(mivi_ctx_t *ctx);
/* One sharded estimate through the RCCL all-reduce route and through the peer-to-peer kernel, every rank collectively; both must agree to 1e-5
 * (value, gradient l2) on EVERY rank (ncclAllReduce(min) of the verdicts).  Only then -- and only with exchange areas of at least one other
 * device attached -- does the automatic route (mivi_comm_set_route 0) take the peer-to-peer kernel at world > 1; until then it is RCCL's
 * reduce-scatter -> mivi_finalize_slice -> all-gather.  rel_out3 (nullable) <- {value rel. difference, gradient rel. l2 difference, 1 if verified}.
 * The reference has no counterpart (single process: src/algorithms/repgradelbo.jl:84-86 is the mean this exchange sums).  A peer-to-peer
 * exchange that does not complete (bounded waits) detaches the areas and returns MIVI_ERR_HIP: the context stays on the RCCL routes. */
mivi_status_t mivi_p2p_selfcheck(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx, double *rel_out3);
/* Batched sharded estimates on the peer-to-peer route run the exchange as ONE persistent kernel on its own stream BESIDE the compute chain
 * (csrc/kernels_p2p.hip), serving groups of four estimates per epoch.  on = 1 (default); 0 = no pipeline: batched calls run serial steps.
 * The pipeline needs the device to schedule the exchange kernel and the compute chain concurrently; where it does not (streams sharing one
 * hardware queue), the bounded waits end in MIVI_ERR_HIP at the next mivi_synchronize -- the host then switches the pipeline off ON EVERY
 * RANK (all ranks must use the same setting). */
mivi_status_t mivi_p2p_set_pipeline(mivi_ctx_t *ctx, int32_t on);
/* developer: the exchange's device words (per lane {epoch, ticket} at 16-word spacing, ready at word 64, freed[ring] at word 80): out128 = uint32[128] */
mivi_status_t mivi_p2p_debug_words(mivi_ctx_t *ctx, uint32_t *out128_host);
/* how many polls (about 1 us each) a wait inside the exchange may take before the peer counts as lost (default 2^21, about 2 s) */
mivi_status_t mivi_p2p_set_spin_budget(mivi_ctx_t *ctx, int32_t polls);
/* Which exchange mivi_estimate_gradient_dist[_n] uses: 0 = automatic (peer-to-peer when attached, otherwise ONE ncclAllReduce + the whole
 * finalisation on every rank below 16 MB of partials and ncclReduceScatter -> slice finalisation -> ncclAllGather -> unpack above),
 * 1 = ncclAllReduce, 2 = ncclReduceScatter / ncclAllGather, 3 = peer-to-peer.  mivi_comm_route reports the route in force. */
mivi_status_t mivi_comm_set_route(mivi_ctx_t *ctx, int32_t route);
int32_t mivi_comm_route(const mivi_ctx_t *ctx);
/* `count` consecutive sharded estimates of the same params (estimates at fixed parameters are independent: the multi-GPU form of
 * mivi_estimate_gradient_n): the exchange + finalisation of estimate t runs on a second stream UNDER the partial kernels of estimate
 * t + 1 (partial vectors double-buffered), one hipGraph per batch; value / grad hold the last estimate on return.  Every rank calls it
 * with the same arguments.  On a batch-engine shape (full-rank f32, d and n_mc multiples of 128 up to 2048, Gaussian target) and routes 1 / 2
 * -- or one rank without peer-to-peer areas -- the batch runs on the batch engine: up to 80 estimates (24 across ranks) per step as one
 * draw / product / VJP launch each, ONE ncclAllReduce per step over all of the step's partial vectors, one finalisation launch; the last
 * estimate then equals `count` single sharded estimates' to rounding (1e-6 value, 2e-6 gradient l2), not bit for bit. */
mivi_status_t mivi_estimate_gradient_dist_n(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx0, int32_t count,
                                            void *value_dev, void *grad_dev);
/* Tests: the phases of the peer-to-peer exchange as separate launches (bit 0 push, bit 1 reduce + finalise, bit 2 unpack), so that
 * several ranks living in ONE process can be sequenced from one host thread.  partials_dev: the rank's partial vector, zero padded. */
mivi_status_t mivi_p2p_exchange(mivi_ctx_t *ctx, const void *params_dev, const void *partials_dev, void *value_dev, void *grad_dev,
                                int32_t phases);
/* Diagnostics of the peer-to-peer exchange since the last reset, one line per rank makes a first multi-GPU run readable: out6[0..2] <- microseconds
 * the exchange kernel (its workgroup 0) waited for {the compute chain's hand-over, the peers' pushes, the owners' reduced chunks}, out6[3] <- groups
 * of estimates served, out6[4] <- payload bytes stored into EACH peer per estimate, out6[5] <- slice length (elements).  reset != 0 zeroes them. */
mivi_status_t mivi_p2p_stats(mivi_ctx_t *ctx, double *out6, int32_t reset);
/* Tests: the partial kernels of one estimate with DIRECT staging -- every entry of the rank's partial vector is stored straight into its
 * owner's staging area (no ring slot, no push pass; what mivi_estimate_gradient_dist[_n] do on the peer-to-peer route for the full-rank f32
 * family); follow with mivi_p2p_exchange(ctx, params, NULL, value, grad, phases).  MIVI_ERR_UNSUPPORTED for other configurations. */
mivi_status_t mivi_p2p_partials_direct(mivi_ctx_t *ctx, const void *params_dev, uint64_t estimate_idx);
/* Measurement (bench.py --gpus N): us per estimate of {partial kernels, exchange + finalisation, the serial step, the pipelined step},
 * hipEvents around one hipGraph replay of `reps` estimates each; every rank calls it collectively.  us_host: double[4]. */
mivi_status_t mivi_profile_dist(mivi_ctx_t *ctx, const void *params_dev, int32_t reps, double *us_host);

/* Measurement hook of the batch engine (kernels_fullrank_batch.hip: what mivi_estimate_gradient_n / _each run for the full-rank family with the
 * diagonal- or dense-Gaussian target): `reps` launches of each of a step's kernels for `lanes` estimates, hipEvents on the context's stream.
 * us_out[0..4] (double[5]) <- average launch duration in microseconds of {draws, product (+ the fused diagonal target), VJP + values, the dense
 * target's product (0 with the diagonal target), the sticking-the-landing product (0 with the other estimators)}.  bench.py's roofline leg. */
mivi_status_t mivi_profile_batch(mivi_ctx_t *ctx, const void *params_dev, int32_t lanes, int32_t reps, double *us_out);
/* Estimates per launch ("lanes" of a step) the batch engine uses for a `count`-estimate call: equal steps of at most 80 lanes. */
int32_t mivi_batch_lanes(const mivi_ctx_t *ctx, int32_t count);
/* What a batch of estimates at this context's configuration runs on (measurement / test hook; the reference has no counterpart: every
 * `estimate_gradient!` there is one AD call, src/algorithms/repgradelbo.jl:151-177).  what = 0: 1 when mivi_estimate_gradient_n / _each with
 * these (16-byte aligned) device parameters take the batch engine, 0 otherwise; 1: matrix-pipe products per 32 x 32 x 16 block of the engine's
 * split-operand contractions (3: f16 hi / lo planes); 2: bytes per operand-plane element (4); 3: 1 once a launch-free optimisation loop's grid-wide
 * exchange was lost on this context (mivi_optimize_loop then restored the caller's state, re-ran the steps on the graph of launches and stays there);
 * 4: the number of hipGraphs recorded into the context's graph cache so far -- unchanged across two calls means the second one replayed;
 * 5: the number of device allocations the library holds right now in this process, over all contexts (the library's one allocate / free pair
 * counts them): equal before a context's creation and after its mivi_destroy means the context returned every allocation it made;
 * 6: the number of HIP streams, events and graph execs the library holds right now in this process, over all contexts (the caller's stream
 * is not one of them; every one sits in an owner that counts its creation and its destruction): the same equality means the context
 * destroyed every handle it created, the children's, the exchange pipelines' and the cached graph included;
 * 7: the route the last mivi_optimize_loop / _batches call on this context ran on -- 0: the graph of launches, else the launch-free loop in
 * the library's priority order (first match): 1 mean-field Descent / default Adam, 2 small logistic regression, 3 mean-field, every other
 * rule x operator x averager, 4 small full-rank in one workgroup, 5 full-rank row-owning workgroups, 6 mean-field fused funnel;
 * after mivi_optimize_loop_many: 16 | the id of the loop whose kernel ran the runs (18 small logistic regressions, 20 small full-rank runs). */
int32_t mivi_batch_info(const mivi_ctx_t *ctx, const void *params_dev, int32_t what);

/* ---- measurement hook (bench.py roofline leg) --------------------------------------------------------- *
 * Times `reps` back-to-back launches of ONE stage of the estimate with hipEvents recorded on the context's
 * stream (after one full warm estimate so every input buffer is populated).
 *   which: 0 = whole estimate, 1 = eps generation, 2 = sample(+fused target) kernel (mean-field: the fused main kernel),
 *          3 = VJP kernel, 4 = dense-target kernel, 5 = the launch-free loop of 100 estimates (mean-field + diagonal
 *          target; what mivi_estimate_gradient_n runs there), 6 / 7 = the split-K product / its reduce kernel alone
 *          (removed), 8 = the sticking-the-landing term W += C^-T eps alone (full-rank, STL estimators),
 *          9 = the LATENCY FLOOR of the full-rank estimate: two empty dependent launches with the grid / block / LDS footprint of the product and VJP kernels,
 *          10 / 11 = the product / VJP launch of FOUR lane-batched estimates (what mivi_estimate_gradient_n issues at the
 *          BASELINE sizes: ms_per_launch is then the time of four estimates' stage).  Stages 1-4, 6, 7, 9-11 are captured `reps` times into one hipGraph and the
 *          replay is timed (eager launches of 2-5 us kernels are host-bound); 0 and 5 are eager.  ms_per_launch_host: double[1]. */
mivi_status_t mivi_profile_kernel(mivi_ctx_t *ctx, int32_t which, const void *params_dev, int32_t reps,
                                  double *ms_per_launch_host);

/* Which kernels the full-rank f32 path runs for `n_samples` per launch on this context (measurement / documentation hook):
 *   bits 0-1: 0 = first generation (32x32 tiles fed from L2, any shape), 1 = unsplit 32x32 product with fused target
 *             (k_fr_prod32) + private-wave VJP (k_fr_vjp32), 2 = split-K LDS-staged product + reduce (k_fr_gemm, k_fr_reduce)
 *             + k_fr_vjp32, 3 = unsplit 64x64 product with fused target (k_fr_prod64, shapes with at least as many tiles as CUs)
 *             + k_fr_vjp32 / k_fr_vjp64;   bit 4: products on the bf16 matrix cores with the exact three-way operand split. */
int32_t mivi_fullrank_route(const mivi_ctx_t *ctx, int32_t n_samples);
/* Which kernels the native logistic-regression target's two data contractions run for `n_samples` per launch (same kind of hook):
 *   0 = vector-ALU kernels (small problems, f64); bit 0: matrix cores (two-way f16 splits); bit 1: the logits on prebuilt operand planes of X
 *   (k_lr_logits_planes); bit 2: X^T R on planes too (k_lr_xtr_planes, residual planes straight from the logits kernel).
 *   On a scheduled context (mivi_logreg_set_batch_schedule): 8 alone = the fused minibatch kernel reads the selected batch through the
 *   schedule; bit 4 (16) = the batch is gathered on the device first, the other bits say which kernels then run on the copy. */
int32_t mivi_logreg_kernels(const mivi_ctx_t *ctx, int32_t n_samples);

/* Developer tool: when buf_dev != NULL every workgroup of the main kernels records wall_clock64() stamps
 * (100 MHz) at buf_dev[block*8 + phase].  NULL switches it off.  Not part of the drop-in surface. */
mivi_status_t mivi_debug_timeline(mivi_ctx_t *ctx, void *buf_dev);

/* ---- host-side RNG restatement (no GPU needed; used by the parity tests) ------------------------- */
void mivi_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* raw words of the eps stream for element (i, global m): out[count] for i = i0 .. i0+count-1 */
void mivi_eps_bits_host(uint64_t seed, uint64_t estimate_idx, int32_t d, int64_t m, int32_t i0, int32_t count,
                        uint32_t *out);
/* eps values themselves evaluated on the host with the same formulas: out_f64[count] */
void mivi_eps_host(uint64_t seed, uint64_t estimate_idx, int32_t d, int64_t m, int32_t i0, int32_t count,
                   int32_t dtype, double *out_f64);

#ifdef __cplusplus
}
#endif
#endif /* MIVI_H */

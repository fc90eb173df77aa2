/*
 * dex_amd.h — C ABI of libdexamd.so: MI355X (gfx950) reverse-diffusion sampler for DEX-TTS / GeDEX-TTS.
 *
 * Drop-in boundary for the reference's Diffusion.forward(..., infer=True) hot path
 *   GeDEX-TTS/model/diffusion.py:220-229, DEX-TTS/model/diffusion.py:250-259
 *   -> ablation_sampler (euler|heun, any alpha; discretization vp/ve/iddpm/edm, schedule vp/ve/linear, scaling vp/none,
 *      range overrides, churn)                    GeDEX-TTS/model/edm.py:109-216 (DEX :104-211)
 *   -> EDMPrecond.forward                          model/edm.py:88-98   (one noise level for the batch inside the sampler and in
 *                                                  dex_denoise_once; one per utterance, as EDMLoss draws them, in dex_denoise_batch)
 *   -> DiffusionDenoiser.forward (+DiTMask, TV/TIV adaptors)
 *                                                  GeDEX diffusion.py:168-207, DEX :190-236, model/dit.py:485-525,
 *                                                  DEX-TTS/model/ref_encoder.py:142-179,255-273
 * and for the STFT/mel front-end audio/tools.py:8-15 -> audio/stft.py:159-178,52-81.
 *
 * Conventions: every pointer named *_dev is a DEVICE pointer (HBM) to contiguous fp32 unless stated;
 * all work is enqueued asynchronously on the caller's HIP stream; the library never synchronises the
 * stream inside dex_sample/dex_denoise_once/dex_denoise_batch.  Functions return 0 on success and a negative DexStatus
 * otherwise; nothing throws across the ABI; dex_last_error() gives the message.
 * Ownership: the caller owns inputs, outputs and the workspace; the library owns the context, its
 * packed weight copies (hipMalloc at dex_ctx_finalize) and captured hipGraphs.
 */
#ifndef DEX_AMD_H
#define DEX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DexCtx DexCtx;
typedef void* dex_stream_t; /* hipStream_t */

typedef enum {
    DEX_PENDING = 1,       /* dex_call_status_poll(wait = 0): the stream has not reached the call's status copy yet */
    DEX_OK = 0,
    DEX_ERR_ARG = -1,      /* bad argument / shape (e.g. T % 4 != 0, unknown key, wrong weight shape) */
    DEX_ERR_STATE = -2,    /* call order (weights missing, not finalized) */
    DEX_ERR_HIP = -3,      /* a HIP runtime call failed */
    DEX_ERR_WORKSPACE = -4,/* workspace too small */
    DEX_ERR_HANDOFF = -5,  /* dex_call_status: an in-launch hand-off of the small-batch DiT block timed out; the call's outputs are NaN */
    DEX_ERR_HANDOFF_XCD = -6 /* dex_call_status: a hand-off met its peer on another XCD (outputs NaN); the XCD-local form is now off for the
                              * device, so REPEATING the call succeeds */
} DexStatus;

typedef enum { DEX_VARIANT_GEDEX = 0, DEX_VARIANT_DEX = 1 } DexVariant;
/* Arithmetic of the contractions: fp32 = exact-fp32 MFMA (the reference's arithmetic, the parity mode); bf16 / fp16 = operands
 * rounded to that type on the MFMA, fp32 accumulation, fp32 norms / softmax state / residual streams. */
typedef enum { DEX_PREC_FP32 = 0, DEX_PREC_BF16 = 1, DEX_PREC_FP16 = 2,
               DEX_PREC_FP16X2 = 3    /* fp16 operands with every weight as hi + lo (two MFMAs per product): the fast mode inside the
                                       * fp32-grade sampler bound */
} DexPrecision;
/* ablation_sampler's solver argument (edm.py:107), and DPM-Solver++(2M): a two-step multistep solver that is not in the reference
 * (second order at one network evaluation per step; DexSamplerTables below). */
typedef enum { DEX_SOLVER_EULER = 0, DEX_SOLVER_HEUN = 1, DEX_SOLVER_DPMPP_2M = 2 } DexSolver;

/* The general ablation_sampler (edm.py:109-216): every branch of discretization / schedule / scaling / alpha / range, as fp32 tables
 * the HOST computes in the reference's operation order (dex_tts_amd/edm.py: ablation_tables) and hands over in DEVICE memory (a
 * captured graph reads them at replay).  Row e describes network evaluation e (n_steps rows for Euler, 2 n_steps - 1 for Heun: step
 * i's predictor at t_hat_i, then its corrector at t'_i = t_hat_i + alpha h_i, none on the last step).  Per evaluation the library does
 *     D = c_skip(sigma) x_in + c_out(sigma) F(c_in(sigma) x_in, ln(sigma) / 4)      with x_in = x / s   (edm.py:88-98, 201, 212)
 *     d = A x - Bc D                                                                 (edm.py:202, 213)
 *     Euler / last step:  x_next = x_hat + h d;    Heun predictor:  x' = x_hat + (alpha h) d;
 *     Heun corrector:     x_next = x_hat + h (w0 d_cur + w1 d')                      (edm.py:203-214)
 * every product and sum rounded on its own, like the reference's torch operations.  Each step starts from
 *     x_hat = r x_cur + k noise_i  (edm.py:196; only when DEX_TABLES_CHURN is set),   and the call from x_0 = z c0 (edm.py:189).
 * alpha needs no flag: the predictor's step alpha h and the corrector's weights are table columns.
 *
 * DEX_SOLVER_DPMPP_2M runs through these tables ONLY (tables == NULL is refused, and so is either flag: the solver works in the
 * (x, sigma) frame, s = 1, and fresh noise would invalidate its history).  n_rows = n_steps, and row e of coef_dev reads
 *     [sigma, 1, a, b, c, 0, 0, 0]:      x_next = a x + b D + c D_prev      (every product and sum rounded on its own)
 * with, for h_i = ln(sigma_i / sigma_{i+1}), r_i = h_{i-1} / h_i, e_i = -expm1(-h_i):  a = sigma_{i+1} / sigma_i,
 * b = e_i (1 + 1 / (2 r_i)), c = -e_i / (2 r_i);  the first row is first order (b = e_0, c = 0: D_prev is not read), the last one
 * (sigma -> 0) is (0, 1, 0).  sigma_dev and step_dev (c0 = sigma_0; r = 1, k = 0) keep their meaning. */
enum {
    DEX_TABLES_SCALED = 1,  /* scaling 'vp': the network input x / s is kept in a buffer of its own (s = 1 otherwise: x_in IS x) */
    DEX_TABLES_CHURN = 2    /* some step has r != 1 or k != 0: every step begins with the x_hat update; noise_dev = [n_steps][B,80,T]
                             * draws, or NULL when every k is 0 */
};
#define DEX_TABLE_EVAL_COLS 8   /* coef_dev row: sigma, s, A, Bc, h, alpha h, w0, w1 */
#define DEX_TABLE_STEP_COLS 4   /* step_dev row: r, k, c0 (row 0 only, else 0), 0 */
typedef struct {
    const float* sigma_dev;     /* [n_rows + 1]: sigma(t) of every evaluation (the network's noise level), then 0 */
    const float* coef_dev;      /* [n_rows][DEX_TABLE_EVAL_COLS]: sigma(t); s(t); A = sigma'(t)/sigma(t) + s'(t)/s(t);
                                 * Bc = sigma'(t) s(t)/sigma(t); the step's h = t_next - t_hat; alpha h; w0 = 1 - 1/(2 alpha); w1 = 1/(2 alpha) */
    const float* step_dev;      /* [n_steps][DEX_TABLE_STEP_COLS]: r = s(t_hat)/s(t_cur); k = sqrt(max(sigma(t_hat)^2 - sigma(t_cur)^2, 0))
                                 * s(t_hat) S_noise; c0 = sigma(t_0) s(t_0) */
    int32_t n_rows;             /* must be dex_num_evals(n_steps, solver) */
    uint32_t flags;             /* DEX_TABLES_* */
} DexSamplerTables;

/* Mirrors Diffusion(**cfg.decoder, dit_cfg=cfg.dit): GeDEX diffusion.py:210, dit.py:339-356. */
typedef struct {
    int32_t variant;        /* DexVariant */
    int32_t n_feats;        /* 80 (hard-coded at diffusion.py:226) */
    int32_t dim;            /* decoder.dim (64) */
    int32_t n_stages;       /* len(dim_mults) (2) */
    int32_t dim_mults[4];
    int32_t n_spks;         /* >1 adds the speaker plane (GeDEX-VCTK) */
    int32_t spk_emb_dim;
    float   pe_scale;       /* 1000 */
    int32_t dit_patch, dit_stride, dit_hidden, dit_depth, dit_heads;
    float   dit_mlp_ratio;
    int32_t dit_conv_pos, dit_conv_pos_groups;
} DexConfig;

/* One Diffusion.forward(infer=True) call == ablation_sampler with a given latent z. */
typedef struct {
    int32_t B, T;               /* batch, padded mel frames (T % 4 == 0, model/utils.py:13-17) */
    int32_t n_steps;            /* n_timesteps >= 2 */
    const float* z_dev;         /* [B,80,T] latent = randn/temperature + mu (diffusion.py:227); drawn by the caller */
    const float* mu_dev;        /* [B,80,T] */
    const float* mask_dev;      /* [B,T]   float 0/1 (reference shape [B,1,T]) */
    const float* sigmas_dev;    /* [n_steps+1] fp32 noise levels t_0..t_{N-1}, t_N=0 (edm.py:157,184-185) */
    const float* spk_dev;       /* [B,spk_emb_dim] or NULL */
    /* DEX only (NULL/0 otherwise): */
    const float* const* ref_skips_dev; /* HOST array of 6 device pointers, each [B,mid,Tr] */
    int32_t n_ref, Tr;
    const float* sty_dev;       /* [B,mid,Ts] */
    const int32_t* sty_lengths_dev; /* [B] int32 */
    int32_t Ts;
    float* out_dev;             /* [B,80,T] x_N (unmasked, like edm.py:216) */
    void*  workspace_dev;       /* >= dex_workspace_bytes(...) bytes, 256-B aligned */
    size_t workspace_bytes;
    int32_t use_graph;          /* 1: the whole call (conditioning tables + every network evaluation + the final copy) is captured
                                 * once into a hipGraph, cached under (shapes, solver, precision, stream, every device pointer
                                 * above) and replayed with ONE hipGraphLaunch; needs a non-default stream */
    int32_t solver;             /* DexSolver; 0 = Euler, what Diffusion wires (diffusion.py:216); DEX_SOLVER_DPMPP_2M needs `tables` */
    /* Stochastic sampler, ablation_sampler's S_churn / S_min / S_max / S_noise (edm.py:109,194-196).  Zero-initialised
     * fields = the deterministic sampler the reference wires (S_churn = 0: its per-step randn_like is multiplied by 0). */
    const float* noise_dev;     /* [n_steps][B,80,T]: step i's randn_like(x_cur) draw (the caller owns the RNG); required
                                 * when S_churn > 0, ignored otherwise */
    float S_churn, S_min, S_max, S_noise;   /* S_max <= 0 means +inf; S_noise is used as given when S_churn > 0 */
    /* NULL: the EDM sampler above (edm / linear / none, alpha = 1), bit for bit what it always was.  Otherwise the general
     * ablation_sampler of the tables (the struct is host memory, the tables device memory): sigmas_dev and S_churn .. S_noise are
     * then ignored, and noise_dev is read only under DEX_TABLES_CHURN. */
    const DexSamplerTables* tables;
} DexSampleArgs;

/* One EDMPrecond.forward call (edm.py:88-98): out = c_skip*x + c_out*F(c_in*x, mask, mu, ln(sigma)/4). */
typedef struct {
    DexSampleArgs s;            /* z_dev is ignored; n_steps ignored; tables ignored; sigmas_dev[0] = sigma */
    const float* x_dev;         /* [B,80,T] */
} DexDenoiseArgs;

/* EDMPrecond.forward with a noise level PER UTTERANCE (edm.py:89 sigma.reshape(-1, 1, 1); what EDMLoss.forward calls, edm.py:31-68):
 *     out_dev[b] = c_skip(sigma_b) x_b + c_out(sigma_b) F(c_in(sigma_b) x_b, mask_b, mu_b, ln(sigma_b) / 4, ...)
 * in ONE network evaluation: asynchronous, sigma_dev is never read by the host, nothing synchronises, nothing is allocated.  The
 * conditioning tables hold one row per utterance, so the workspace is dex_workspace_bytes(ctx, B, T, Tr, Ts, n_evals = B).
 * Refused with DEX_ERR_ARG before anything is enqueued: a null x_dev / sigma_dev, B < 1, the shapes dex_denoise_once refuses, and
 * use_graph = 1 (this call is not captured).  The VALUES of sigma_dev are the caller's business, as in the reference: a level that
 * is not positive and finite gives NaN / inf rows, no error.  Taps, profile rows and dex_call_status* treat it as "the LAST call"
 * like dex_denoise_once (the "mlp" and "vit.t_embedder" taps have B rows). */
typedef struct {
    DexSampleArgs s;            /* as in DexDenoiseArgs: z_dev, n_steps, tables, sigmas_dev, solver, churn fields ignored */
    const float* x_dev;         /* [B,80,T] */
    const float* sigma_dev;     /* [B] fp32, DEVICE memory: utterance b's noise level (edm.py:89 sigma.reshape(-1,1,1)) */
} DexDenoiseBatchArgs;

int  dex_ctx_create(const DexConfig* cfg, DexCtx** out);
void dex_ctx_destroy(DexCtx* ctx);
const char* dex_last_error(const DexCtx* ctx);
const char* dex_version(void);

/* Number of state-dict tensors the context expects, and the i-th key (relative to "denoise_fn.") + shape. */
int  dex_ctx_num_weights(const DexCtx* ctx);
int  dex_ctx_weight_info(const DexCtx* ctx, int i, const char** key, int64_t shape[4], int* ndim);
/* Hand over one tensor in the REFERENCE layout (fp32, contiguous, device memory).  The library copies it into its own
 * HBM before returning control of the pointer:
 *   dex_ctx_load_weight        synchronous — the copy runs on the legacy null stream and has completed on return; the
 *                              caller must have completed whatever produced w_dev (it is NOT ordered against
 *                              non-blocking streams);
 *   dex_ctx_load_weight_async  the copy is enqueued on `stream`, i.e. ordered after the kernels that produced w_dev on
 *                              that stream; w_dev must stay valid until the stream reaches the copy (dex_ctx_finalize on
 *                              the same stream synchronises it). */
int  dex_ctx_load_weight(DexCtx* ctx, const char* key, const float* w_dev, const int64_t* shape, int ndim);
int  dex_ctx_load_weight_async(DexCtx* ctx, const char* key, const float* w_dev, const int64_t* shape, int ndim,
                               dex_stream_t stream);
/* Pack all weights into kernel layouts (library-owned HBM) on `stream` and wait for it on the host before returning:
 * after dex_ctx_finalize the packed weights are complete for work on ANY stream. */
int  dex_ctx_finalize(DexCtx* ctx, dex_stream_t stream);
int  dex_ctx_set_precision(DexCtx* ctx, int precision /* DexPrecision */);

/* n_evals = number of network evaluations of the run: dex_num_evals(n_steps, solver); for dex_denoise_batch: B. */
size_t dex_workspace_bytes(const DexCtx* ctx, int B, int T, int Tr, int Ts, int n_evals);
/* Euler and DPM-Solver++(2M): n_steps.  Heun (edm.py:202-214): 2*n_steps - 1 (no corrector on the last step). */
int  dex_num_evals(int n_steps, int solver /* DexSolver */);
int  dex_sample(DexCtx* ctx, const DexSampleArgs* args, dex_stream_t stream);
int  dex_denoise_once(DexCtx* ctx, const DexDenoiseArgs* args, dex_stream_t stream);
int  dex_denoise_batch(DexCtx* ctx, const DexDenoiseBatchArgs* args, dex_stream_t stream);

/* EDM rho=7 schedule in fp32 on the host (edm.py:157): writes n_steps+1 values, last one 0. */
int  dex_edm_sigmas(int n_steps, float* sigmas_host);

/* Debug taps: copy a named intermediate of the LAST dex_denoise_once/dex_denoise_batch/dex_sample call out of the
 * workspace (device->device, async on stream).  Names: see dex_tap_name(i).  Layout NHWC fp32. */
int  dex_num_taps(const DexCtx* ctx);
const char* dex_tap_name(const DexCtx* ctx, int i);
int  dex_tap_info(const DexCtx* ctx, const char* name, int64_t shape[4], int* ndim);
int  dex_tap_copy(DexCtx* ctx, const char* name, float* dst_dev, size_t dst_bytes, dex_stream_t stream);

/* Per-kernel timing of the last dex_sample with profiling enabled (HIP events on the launch stream). */
int  dex_profile_enable(DexCtx* ctx, int on);
int  dex_profile_num(const DexCtx* ctx);
int  dex_profile_get(const DexCtx* ctx, int i, const char** name, int* calls, double* total_ms,
                     double* flops, double* bytes);

/* Status of the LAST dex_sample / dex_denoise_once call of this context on `stream`.  Small-grid DiT blocks run as clusters of
 * co-operating workgroups whose in-launch hand-offs are bounded waits: a lost hand-off cannot hang the GPU, it turns every output of
 * the call into NaN and sets a device word.  This call waits for the stream and reads that word: DEX_OK, DEX_ERR_HANDOFF (a
 * time-out) or DEX_ERR_HANDOFF_XCD (a peer on another XCD) - the outputs are NaN in both.  In the second case the XCD-local form is
 * switched off for the device - for every context - so repeating the call succeeds.  A hipGraph replay is checked like an eager call
 * (the graph entry remembers the word its captured launches write).  Calls that used no hand-offs return DEX_OK without waiting.  The Python mirror
 * (ScoreNetEngine.sample) checks every call that could use hand-offs and raises. */
int  dex_call_status(DexCtx* ctx, dex_stream_t stream);
/* The same verdict WITHOUT blocking the host (the sampler call is asynchronous: a caller overlaps the vocoder of utterance i with the
 * sampler of utterance i + 1).  _begin enqueues, behind the last dex_sample / dex_denoise_once on `stream`, a copy of the call's
 * hand-off word into a pinned host word of the context and an event; it returns at once (calls without hand-offs: nothing is enqueued).
 * _poll returns the verdict of that call - DEX_OK / DEX_ERR_HANDOFF / DEX_ERR_HANDOFF_XCD - once the event has passed; before that
 * DEX_PENDING (wait = 0), or it waits for that event alone (wait != 0; never for later work on the stream).  One check is in flight per
 * context: a second _begin first resolves the pending one (and returns its error if it failed).  The Python mirror's default
 * (ScoreNetEngine.check_handoffs = "deferred") begins a check after every call and reads it at the next call or at .status(). */
int  dex_call_status_begin(DexCtx* ctx, dex_stream_t stream);
int  dex_call_status_poll(DexCtx* ctx, int wait);
/* Debug: 1 if a workgroup hand-off of the LAST dex_sample / dex_denoise_once call on this context timed out (small-grid DiT
 * blocks run as clusters of co-operating workgroups; a wait is bounded so a lost hand-off cannot hang the GPU), 0 if none did or
 * the call used no hand-offs, < 0 on a HIP error.  Synchronises the stream; the call's workspace must still be alive. */
int  dex_debug_handoff_timeouts(DexCtx* ctx, dex_stream_t stream);
/* Debug: 1 if workgroup b of a launch runs on XCD b % 8 on this device (probed once per process with launches that record
 * HW_REG_XCC_ID), which lets the clusters above keep their hand-offs inside one XCD's L2; 0 if not (or DEX_DIT_CLUSTER_LOCAL=0):
 * the hand-offs then go through memory.  Every hand-off of the XCD-local form re-checks its peers' XCC ids; a mismatch poisons the
 * call like a time-out (dex_debug_handoff_timeouts returns 2 and switches the form off for the process). */
int  dex_debug_xcd_local(void);

/* STFT/mel front-end (audio/tools.py:8-15): wav [L] fp32 in [-1,1] (clipped here) -> mel [80,frames],
 * energy [frames]; frames = L/256 + 1.  n_fft=1024, hop=256, 80 mels, 22050 Hz, fmin 0, fmax 8000. */
int  dex_mel_frames(int n_samples);
int  dex_mel_from_wav(DexCtx* ctx, const float* wav_dev, int n_samples, float* mel_dev, float* energy_dev,
                      dex_stream_t stream);

/* The same front-end without a score-network context and for a batch — replaces TacotronSTFT.mel_spectrogram(y [B,L])
 * (audio/stft.py:159-178, called by preprocess/preprocessor/preprocessor.py:100 and audio/tools.py:8-15): B equally long rows
 * in ONE pass (pad/clip kernel, one batched windowed-DFT GEMM, one magnitude/mel/log kernel).  wav [B,L] fp32 (clipped to
 * [-1,1] here) -> mel [B,80,frames], energy [B,frames]; the caller owns the workspace (dex_mel_workspace_bytes). */
typedef struct DexMel DexMel;
int  dex_mel_create(DexMel** out);
void dex_mel_destroy(DexMel* mel);
const char* dex_mel_last_error(const DexMel* mel);
size_t dex_mel_workspace_bytes(int B, int n_samples);
int  dex_mel_spectrogram(DexMel* mel, const float* wav_dev, int B, int n_samples, float* mel_dev, float* energy_dev,
                         void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);

/* Deterministic tail of the DEX f0 front-end (DEX-TTS/synthesize.py:26-38,55-58): f0 [B,T] in Hz (0 = unvoiced; from
 * dex_f0_dio + dex_f0_stonemask below, or from any other tracker) -> lf0 [B,T] = normalize_lf0(log f0), what
 * dex_style_encode takes as lf0_dev.  lengths_dev [B] int32 or NULL (= T); positions past an utterance's length are 0.
 * T <= 16382 frames (190 s of audio at hop 256): DEX_ERR_ARG beyond. */
int  dex_lf0_normalize(const float* f0_dev, const int* lengths_dev, int B, int T, float* lf0_dev, dex_stream_t stream);

/* ---- f0 tracker (DEX-TTS/synthesize.py:46-52): WORLD's DIO + StoneMask (M. Morise) on the device, for a ragged batch.  The
 * contract is the docstring of tests/world_f0.py; parity with pyworld itself is NOT measured (pyworld is not available to this
 * project): the kernels are held to that float64 restatement and to signals whose f0 is known analytically.  speed = 1 only (no
 * decimation).  All arithmetic fp64 in a fixed order: a row's result is bitwise reproducible and independent of its batch.
 * wav_dev [B, n_samples] fp32 (promoted to fp64 exactly); row b holds lengths_host[b] samples (a HOST array, each in
 * [1, n_samples]).  Frame i lies at t = i * frame_period_ms / 1000; row b has F(lengths_host[b]) frames, F(L) =
 * int(1000 L / fs / frame_period_ms) + 1.  Bad arguments return DEX_ERR_ARG before anything is enqueued. */
typedef struct { double fs, frame_period_ms, f0_floor, f0_ceil, channels_in_octave, allowed_range; } DexF0Opts;  /* NULL = DEX's: 22050, 256/22050*1000, 71, 800, 2, 0.1 */
int    dex_f0_frames(int n_samples, const DexF0Opts* opts);          /* host only: F of the contract; DEX_ERR_ARG for bad options */
size_t dex_f0_workspace_bytes(int B, const int* lengths_host, const DexF0Opts* opts);   /* for dex_f0_dio; 0 for bad arguments */
/* synthesize.py:46: out [B, n_samples] = float(x / max|x|) per row, computed in fp64 (0 past a row's length, and for a silent row). */
int    dex_f0_peak_normalize(const float* wav_dev, const int* lengths_host, int B, int n_samples, float* out_dev, dex_stream_t s);
/* pw.dio(x, fs, f0_floor, f0_ceil, channels_in_octave, frame_period, speed = 1, allowed_range) -> f0_dev [B, F(n_samples)] fp64,
 * 0 past each row's F.  The workspace holds the per-row filter outputs and events (about (2 + 3 nb) max(L) doubles per row, nb = 7 bands by default). */
int    dex_f0_dio(const float* wav_dev, const int* lengths_host, int B, int n_samples, const DexF0Opts* opts,
                  double* f0_dev /* [B, F(n_samples)], 0 past each utterance's F */, void* ws, size_t ws_bytes, dex_stream_t s);
/* pw.stonemask(x, f0, t, fs) with t the frame times above: f0_in_dev / f0_out_dev [B, F(n_samples)] fp64 (distinct buffers).
 * Needs no workspace (ws may be NULL). */
int    dex_f0_stonemask(const float* wav_dev, const int* lengths_host, int B, int n_samples, const DexF0Opts* opts,
                        const double* f0_in_dev, double* f0_out_dev, void* ws, size_t ws_bytes, dex_stream_t s);

/* ---- Reference wav preparation (DEX-TTS/synthesize.py:40-47, ahead of the f0 tracker): librosa.effects.trim(top_db = 30),
 * resampy.resample(kaiser_best) to 22050 Hz and the fp64 peak normalisation, for a ragged, mixed-rate batch.  The contract is the
 * docstring of tests/wav_prep.py; parity with librosa 0.9.2 and resampy themselves is NOT measured (neither is available to this
 * project).  fp64 throughout, every reduction in a fixed order: a row's result is bitwise reproducible and independent of its batch.
 * Row lengths, offsets and rates are HOST arrays; bad arguments return DEX_ERR_ARG before anything is enqueued. */
enum { DEX_WAV_PAD_CONSTANT = 0, DEX_WAV_PAD_REFLECT = 1 };
typedef struct {
    double top_db;                    /* 30: a frame is non-silent iff 10 log10(mse / max mse) > -top_db (both floored at 1e-10) */
    int32_t frame_length, hop_length; /* 2048, 512; frame_length must be a multiple of hop_length */
    int32_t pad_mode;                 /* DEX_WAV_PAD_CONSTANT (zeros) or DEX_WAV_PAD_REFLECT (numpy "reflect"), frame_length / 2 each side */
} DexWavTrimOpts;                     /* NULL = 30, 2048, 512, constant */
typedef struct {
    int32_t num_zeros, precision;     /* 64, 9: the table has 2^precision * num_zeros + 1 entries */
    double beta, rolloff;             /* kaiser window beta 14.769656459379492, rolloff 0.9475937167399596 */
} DexWavResampleOpts;                 /* NULL = resampy's kaiser_best */
/* wav_dev [B, n_samples] fp32 (promoted exactly) -> bounds_dev [B, 2] int32 (start, end) of the non-silent part of each row; optional
 * frame_mse_dev [B, 1 + n_samples / hop_length] fp64 (NULL: not written): each frame's mean square, 0 past a row's 1 + L / hop frames. */
size_t dex_wav_trim_workspace_bytes(int B, const int* lengths_host, const DexWavTrimOpts* opts);   /* 0 for bad arguments */
int    dex_wav_trim(const float* wav_dev, const int* lengths_host, int B, int n_samples, const DexWavTrimOpts* opts, int32_t* bounds_dev,
                    double* frame_mse_dev, void* ws, size_t ws_bytes, dex_stream_t s);
/* host only: (n_samples * sr_new) div sr_orig, DEX_ERR_ARG if a rate is <= 0, n_samples < 1, or the result is < 1 or above INT32_MAX */
int    dex_wav_resampled_length(int n_samples, int sr_orig, int sr_new);
/* The window table (2^precision * num_zeros + 1 pairs of doubles, 16-byte aligned): built once on the device by dex_wav_resample_table,
 * then read by every dex_wav_resample call made with the same options. */
size_t dex_wav_resample_table_bytes(const DexWavResampleOpts* opts);                             /* 0 for bad options */
int    dex_wav_resample_table(const DexWavResampleOpts* opts, void* table_dev, size_t table_bytes, dex_stream_t s);
/* Row b reads wav_dev[b * in_stride + offsets_host[b] ...] for lengths_host[b] samples at sr_orig_host[b] Hz and writes
 * dex_wav_resampled_length(...) fp64 samples at sr_new to out_dev[b * out_stride ...], 0 up to out_stride.  A row already at sr_new
 * is copied.  sr_new / sr_orig must be >= 1 / 2^precision. */
int    dex_wav_resample(const float* wav_dev, int in_stride, const int* offsets_host, const int* lengths_host, const int* sr_orig_host,
                        int B, int sr_new, const DexWavResampleOpts* opts, double* out_dev, int out_stride, const void* table_dev,
                        size_t table_bytes, dex_stream_t s);
/* synthesize.py:46 on fp64 rows: out [B, n_samples] fp32 = float(x / max|x|) per row (0 past a row's length and for a silent row). */
size_t dex_wav_peak_workspace_bytes(int B, int n_samples);                                        /* 0 for bad arguments */
int    dex_wav_peak_normalize_f64(const double* x_dev, const int* lengths_host, int B, int n_samples, float* out_dev, void* ws,
                                  size_t ws_bytes, dex_stream_t s);

/* ---- Vocoder: HiFi-GAN generator (GeDEX-TTS/hifigan/models.py:112-173, built by src/utils.py:251-281 from
 * hifigan/config.json) — the step right after the sampler: mel [B,80,T] -> waveform [B, T * prod(upsample_rates)].
 * A separate context: it shares nothing with the score network. */
typedef struct DexVoc DexVoc;
typedef struct {
    int32_t num_mels;                   /* 80 */
    int32_t upsample_initial_channel;   /* 512 (V1) */
    int32_t n_upsamples;                /* len(upsample_rates), <= 6 */
    int32_t upsample_rates[6];          /* [8,8,2,2] */
    int32_t upsample_kernel_sizes[6];   /* [16,16,4,4] */
    int32_t n_resblock_kernels;         /* len(resblock_kernel_sizes), must be 3 (the stage average is xs / 3) */
    int32_t resblock_kernel_sizes[3];   /* [3,7,11] */
    int32_t resblock_dilation_sizes[3][3]; /* [[1,3,5]]*3 (ResBlock "1": three dilated + three plain convs each) */
    /* 0: HiFi-GAN (leaky_relu in front of every conv).  1 / 2: BigVGAN (DEX-TTS/bigvgan/models.py:138-211, AMPBlock1) with the
     * anti-aliased Snake / SnakeBeta activation (alias_free_torch/act.py, activations.py) in front of every ResBlock conv and of
     * conv_post, and no activation in front of the transposed convs. */
    int32_t activation;
    int32_t snake_logscale;             /* BigVGAN: alpha / beta are stored as logarithms (config "snake_logscale") */
} DexVocoderConfig;

int  dex_voc_create(const DexVocoderConfig* cfg, DexVoc** out);
void dex_voc_destroy(DexVoc* voc);
const char* dex_voc_last_error(const DexVoc* voc);
/* Generator.state_dict() keys AFTER remove_weight_norm() (models.py:169-173: "conv_pre.weight", "ups.0.bias",
 * "resblocks.4.convs1.2.weight", "conv_post.weight", ...), reference shapes; the host folds weight_g / weight_v pairs.
 * BigVGAN: "ups.<i>.0.weight" (nested ModuleList), "resblocks.<n>.activations.<l>.act.alpha" [+ ".beta"],
 * "activation_post.act.alpha" [+ ".beta"], and ONE copy of the two (identical) 12-tap resampling filters,
 * "activation_post.upsample.filter" / "activation_post.downsample.lowpass.filter" [1,1,12]. */
int  dex_voc_num_weights(const DexVoc* voc);
int  dex_voc_weight_info(const DexVoc* voc, int i, const char** key, int64_t shape[4], int* ndim);
int  dex_voc_load_weight_async(DexVoc* voc, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream);
int  dex_voc_finalize(DexVoc* voc, dex_stream_t stream);
size_t dex_voc_workspace_bytes(const DexVoc* voc, int B, int T);
int  dex_voc_samples(const DexVoc* voc, int T);          /* T * prod(upsample_rates) */
/* Operand precision of the generator's convolutions (DexPrecision): DEX_PREC_FP32 (default; exact-fp32 MFMA, the parity mode) or
 * DEX_PREC_BF16 / DEX_PREC_FP16 (operands rounded while staged, fp32 accumulation, fp32 activations in HBM, weights packed for
 * both at dex_voc_finalize).  Takes effect at the next dex_vocode. */
int  dex_voc_set_precision(DexVoc* voc, int precision);
/* Generator.forward (models.py:150-167): mel_dev [B,num_mels,T] fp32 -> wav_dev [B, dex_voc_samples(T)] fp32 in [-1,1].
 * Exact-fp32 MFMA contractions (the reference's arithmetic).  Asynchronous on `stream`. */
int  dex_vocode(DexVoc* voc, const float* mel_dev, int B, int T, float* wav_dev, void* workspace_dev, size_t workspace_bytes,
                dex_stream_t stream);
/* Ragged batches: utterance b is vocoded exactly as if it had been passed alone at lengths_dev[b] frames - at every layer its sequence
 * ends at lengths_dev[b] * R samples (R = the layer's cumulative up-sampling rate: zero padding for the convolutions, the anti-aliased
 * activations' replicate padding from its own last sample) - and wav_dev[b, lengths_dev[b] * hop:] is exactly zero.  The content of
 * mel_dev past an utterance's length is ignored (NaN included).  lengths_dev: B int32 frame counts ON THE DEVICE, each clamped to
 * [0, T] by the kernels; nothing is copied to the host and nothing synchronises.  lengths_dev == NULL: every utterance is T frames
 * long, the result is dex_vocode's.  Needs dex_voc_ragged_workspace_bytes (>= dex_voc_workspace_bytes; 0 for B < 1 or T < 1). */
size_t dex_voc_ragged_workspace_bytes(const DexVoc* voc, int B, int T);
int  dex_vocode_ragged(DexVoc* voc, const float* mel_dev, const int32_t* lengths_dev, int B, int T, float* wav_dev, void* workspace_dev,
                       size_t workspace_bytes, dex_stream_t stream);
/* Windowed calls: long utterances in bounded memory, audio handed out as it is computed.  The generator has a finite receptive field:
 * with dex_voc_halo_frames() = H frames of context on each side, the samples of the frames [t0, t0 + n_frames) depend on nothing outside
 * [t0 - H, t0 + n_frames + H).  H follows from the configuration alone (kernel sizes, dilations, rates, the resampling filters' lengths);
 * it is valid right after dex_voc_create.
 * dex_vocode_window writes, for every utterance b, the samples [t0 * hop, (t0 + n_frames) * hop) that dex_vocode_ragged(mel_dev,
 * lengths_dev, B, T) writes - in fp32 bit for bit - to wav_dev[b * wav_bstride + 0 .. n_frames * hop): a pointer t0 * hop samples into
 * the full [B, T * hop] waveform with wav_bstride = T * hop assembles the whole result in place.  lengths_dev == NULL: every utterance
 * has T frames (dex_vocode's result); samples past lengths_dev[b] * hop are exactly zero.  mel_dev [B,num_mels,T] is read only in the
 * frames [max(0, t0 - H), min(T, t0 + n_frames + H)) and, of those, below each utterance's length.  Asynchronous on `stream`; nothing is
 * copied to the host.  DEX_ERR_ARG, with nothing enqueued, for t0 < 0, n_frames < 1, t0 + n_frames > T, B < 1, wav_bstride <
 * n_frames * hop, or a workspace below dex_voc_window_workspace_bytes(B, n_frames) - which does not depend on T (0 for B < 1 or
 * n_frames < 1). */
int    dex_voc_halo_frames(const DexVoc* voc);
size_t dex_voc_window_workspace_bytes(const DexVoc* voc, int B, int n_frames);
int    dex_vocode_window(DexVoc* voc, const float* mel_dev, const int32_t* lengths_dev, int B, int T, int t0, int n_frames, float* wav_dev,
                         int64_t wav_bstride, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);

/* ---- DEX style encoders (DEX-TTS/model/ref_encoder.py TVEncoder :110-140 + VQEmbeddingEMA :199-237, LF0Encoder
 * :36-55, TIVEncoder :83-108, DeXTTS.conv_sty tts.py:31) and the part of DeXTTS.forward that feeds the decoder (tts.py:55-66):
 * the step right before the sampler for the DEX configs, once per reference utterance.  Eval mode (dropout off, BatchNorm on
 * running statistics — folded into the convolutions by the caller —, frozen codebook).  A separate context. */
typedef struct DexStyle DexStyle;
typedef struct {
    int32_t n_mels;                                             /* 80 */
    int32_t tiv_layers, tiv_ch;                                 /* tiv_encoder: num_layer 6, c_h 128 (skips [B,c_h,Tr]) */
    int32_t tv_layers, tv_ch, tv_cout, tv_cout_g, tv_n_emb;     /* tv_encoder: 6, 128, 192, 192, 512 */
    int32_t lf0_ch, lf0_cout, lf0_cout_g, lf0_layers;           /* lf0_encoder: 192, 192, 192, 2 (GRU hidden = lf0_ch / 2 = 96) */
    int32_t sty_out;                                            /* conv_sty output channels = 2 * decoder.dim (128) */
} DexStyleConfig;
typedef struct {
    int32_t B, Tr, Ts, Tl;
    const float* ref_mel_dev;  const int32_t* ref_lengths_dev;  /* [B,n_mels,Tr], [B]  -> TIVEncoder */
    const float* sty_mel_dev;  const int32_t* sty_lengths_dev;  /* [B,n_mels,Ts], [B]  -> TVEncoder  */
    const float* lf0_dev;      const int32_t* lf0_lengths_dev;  /* [B,Tl], [B]         -> LF0Encoder (normalised log-f0, 0 = unvoiced) */
    float* const* ref_skips_out_dev;   /* HOST array of tiv_layers device pointers, each [B,tiv_ch,Tr]: Diffusion.forward's `ref` */
    float* sty_dec_out_dev;            /* [B,sty_out,Ts]: Diffusion.forward's `sty` (conv_sty(z_dec + mean lf0_dec)) */
    float* sty_enc_out_dev;            /* [B,tv_cout]: pooled style vector for the text encoder (tts.py:62-63) */
    int32_t* vq_idx_out_dev;           /* optional [B,Ts]: the chosen codebook rows */
    void* workspace_dev; size_t workspace_bytes;
} DexStyleArgs;

int  dex_style_create(const DexStyleConfig* cfg, DexStyle** out);
void dex_style_destroy(DexStyle* sty);
const char* dex_style_last_error(const DexStyle* sty);
/* Keys = the reference state-dict names under tv_encoder.* / lf0_encoder.* / tiv_encoder.* / conv_sty.*; a conv followed by
 * BatchNorm is handed over FOLDED as "<p>.conv.weight" + "<p>.conv.bias" (dex_tts_amd/style.py does it). */
int  dex_style_num_weights(const DexStyle* sty);
int  dex_style_weight_info(const DexStyle* sty, int i, const char** key, int64_t shape[4], int* ndim);
int  dex_style_load_weight_async(DexStyle* sty, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream);
int  dex_style_finalize(DexStyle* sty, dex_stream_t stream);
size_t dex_style_workspace_bytes(const DexStyle* sty, int B, int Tr, int Ts, int Tl);
int  dex_style_encode(DexStyle* sty, const DexStyleArgs* args, dex_stream_t stream);
/* dex_style_encode plus the eval-mode VQ commitment loss of VQEmbeddingEMA.forward (ref_encoder.py:226) as a 0-d fp32 on the
 * device: vq_loss_out_dev[0] = commit_w * sum (x m - e[idx] m)^2 / (sum m * tv_cout), x = z_beforeVQ [B,Ts,tv_cout], m the sty mask.
 * Every output of dex_style_encode is bitwise the same.  Per-row fp64 partials in a fixed order, one combine, no atomics: the
 * same bits on every run.  The workspace must hold dex_style_loss_workspace_bytes. */
size_t dex_style_loss_workspace_bytes(const DexStyle* sty, int B, int Tr, int Ts, int Tl);
int  dex_style_encode_loss(DexStyle* sty, const DexStyleArgs* args, float commit_w, float* vq_loss_out_dev, dex_stream_t stream);

/* ---- Text encoder + durations + alignment: TextEncoder.forward (GeDEX-TTS/model/text_encoder.py:129-146, DEX
 * :126-142: embedding, ConvReluNorm prenet, RetNet in its parallel form with use_softmax = True / use_decay = False — the only
 * setting the shipped configs use —, proj_m, DurationPredictor) and the lines of the TTS forward between the encoder and the
 * decoder (tts.py:37-50: w_ceil, y_lengths, generate_path, mu_y).  Once per utterance; exact-fp32 arithmetic.  Eval mode. */
typedef struct DexText DexText;
typedef struct {
    int32_t variant;                  /* DEX_VARIANT_GEDEX, or DEX_VARIANT_DEX: AdaptiveLayerNorm(sty) after both residual sums of every layer */
    int32_t n_vocab, n_feats, n_channels, filter_channels, filter_channels_dp, n_heads, n_layers, kernel_size;
    int32_t n_spks, spk_emb_dim;      /* n_spks > 1: the speaker embedding is concatenated to the prenet output (RetNet width n_channels + spk_emb_dim) */
    int32_t use_softmax, use_decay;   /* must be 1, 0 */
} DexTextConfig;
typedef struct {
    int32_t B, T;
    const int32_t* tokens_dev;        /* [B,T] token ids */
    const int32_t* lengths_dev;       /* [B], each in [1, T] */
    const float* spk_dev;             /* [B,spk_emb_dim] speaker embedding rows (spk_emb(spk), tts.py:31) when n_spks > 1, else NULL */
    const float* sty_dev;             /* [B,n_channels] pooled style vector (dex_style_encode's sty_enc) for DEX_VARIANT_DEX, else NULL */
    float length_scale;               /* tts.py:38 */
    float* mu_out_dev;                /* [B,n_feats,T]  mu_x */
    float* logw_out_dev;              /* [B,T]          log durations */
    float* w_ceil_out_dev;            /* [B,T]          ceil(exp(logw) * mask) * length_scale */
    int32_t* y_lengths_out_dev;       /* [B]            clamp_min(sum w_ceil, 1) as integers: read these to size the alignment */
    void* workspace_dev; size_t workspace_bytes;
} DexTextArgs;
typedef struct {
    int32_t B, T, Ty;                 /* Ty = fix_len_compatibility(max y_lengths) */
    const float* mu_x_dev;            /* [B,n_feats,T] */
    const float* w_ceil_dev;          /* [B,T] */
    const int32_t* x_lengths_dev;     /* [B] */
    const int32_t* y_lengths_dev;     /* [B] */
    float* mu_y_out_dev;              /* [B,n_feats,Ty] = attn^T mu_x  (the decoder's mu) */
    float* y_mask_out_dev;            /* [B,Ty] */
    float* attn_out_dev;              /* optional [B,T,Ty] 0/1 alignment (generate_path) */
    void* workspace_dev; size_t workspace_bytes;     /* >= B*T floats */
} DexAlignArgs;

int  dex_text_create(const DexTextConfig* cfg, DexText** out);
void dex_text_destroy(DexText* txt);
const char* dex_text_last_error(const DexText* txt);
/* Keys = the reference TextEncoder state-dict names (emb.weight, prenet.*, encoder.layers.<i>.*, encoder.layer_norm.weight,
 * encoder.retnet_rel_pos.angle, proj_m.*, proj_w.*); encoder.retnet_rel_pos.decay is not used (use_decay = 0). */
int  dex_text_num_weights(const DexText* txt);
int  dex_text_weight_info(const DexText* txt, int i, const char** key, int64_t shape[4], int* ndim);
int  dex_text_load_weight_async(DexText* txt, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream);
int  dex_text_finalize(DexText* txt, dex_stream_t stream);
size_t dex_text_workspace_bytes(const DexText* txt, int B, int T);
int  dex_text_encode(DexText* txt, const DexTextArgs* args, dex_stream_t stream);
int  dex_text_align(DexText* txt, const DexAlignArgs* args, dex_stream_t stream);

/* ---- Monotonic alignment search (Glow-TTS MAS) and the validation losses around it: the log-prior of compute_loss (GeDEX-TTS/model/
 * tts.py:75-80, DEX :99-106), model.monotonic_align.maximum_path with the reference's exact fp32 semantics (value * mask, the -1e9
 * sentinel, strict comparison in the backtrack) and the duration / prior loss reductions (tts.py:112-113, :148-149).  Lengths are HOST
 * arrays; every bad argument, a row with t_y < t_x among them, is refused before anything is enqueued.  The result of a row does not
 * depend on the other rows of its batch. */
#define DEX_MAS_MAX_TX 2048
#define DEX_MAS_MAX_TY 8192
/* log_prior[b, y, x] ([B,Ty,Tx], frame-major: the layout the search reads) from mu_x [B,n_feats,Tx] and y [B,n_feats,Ty]; n_feats <= 128. */
int    dex_mas_log_prior(const float* mu_x_dev, const float* y_dev, int B, int n_feats, int Tx, int Ty, float* log_prior_dev, dex_stream_t s);
size_t dex_mas_workspace_bytes(int B, int Tx, int Ty);   /* 0 for bad arguments */
/* value[b, x, y] at value_dev + b stride_b + x stride_x + y stride_y (element strides; mask_dev, optional, has the same strides and
 * multiplies value first).  Row b searches the t_x = x_lengths_host[b] by t_y = y_lengths_host[b] corner, 1 <= t_x <= t_y.
 * dur_dev [B,Tx] int32: frames per token (0 past t_x).  path_dev: optional dense [B,Tx,Ty] 0/1 path. */
int    dex_mas_durations(const float* value_dev, const float* mask_dev, int B, int Tx, int Ty, int64_t stride_b, int64_t stride_x,
                         int64_t stride_y, const int* x_lengths_host, const int* y_lengths_host, int32_t* dur_dev, float* path_dev,
                         void* workspace_dev, size_t workspace_bytes, dex_stream_t s);
size_t dex_mas_loss_workspace_bytes(int B);              /* 0 for bad arguments */
/* out_dev[0] = dur_loss = sum (logw - log(1e-8 + dur) x_mask)^2 / sum x_lengths, logw / dur [B,Tx];
 * out_dev[1] = prior_loss = sum 0.5 ((y - mu_y)^2 + log 2 pi) y_mask / (sum y_mask n_feats), y / mu_y [B,n_feats,Ty].
 * Per-utterance partial sums in a fixed order, then one combine on the device: nothing is read back. */
int    dex_mas_losses(const float* logw_dev, const int32_t* dur_dev, const int* x_lengths_host, int B, int Tx, const float* y_dev,
                      const float* mu_y_dev, const int* y_lengths_host, int n_feats, int Ty, float* out_dev, void* workspace_dev,
                      size_t workspace_bytes, dex_stream_t s);

/* ---- Segment expand + cut of compute_loss (tts.py:115-144): from mu_x [B,n_feats,Tx], the search's durations dur [B,Tx] int32
 * and y [B,n_feats,Ty], for t < cut_b = min(S, y_lengths_host[b]):
 *     y_cut[b, :, t] = y[b, :, off_b + t],  mu_y_cut[b, :, t] = mu_x[b, :, k] with sum(dur[b, :k]) <= off_b + t < sum(dur[b, :k+1]),
 *     y_cut_mask[b, 0, t] = 1;   every output is 0 for t >= cut_b (and mu_y_cut where no token owns the frame).
 * y_cut / mu_y_cut [B,n_feats,S], y_cut_mask [B,1,S].  S = out_size for a cut, Ty for none; offsets_host NULL = all 0; each
 * 0 <= off_b <= y_lengths_host[b] - cut_b.  mu_y_cut is bitwise the reference's attn_cut^T mu_x.  Tx <= DEX_MAS_MAX_TX,
 * Ty <= DEX_MAS_MAX_TY.  Bad arguments are refused before anything is enqueued; a row's result does not depend on its batch. */
int    dex_loss_segment(const float* mu_x_dev, const int32_t* dur_dev, const float* y_dev, int B, int n_feats, int Tx, int Ty,
                        const int* y_lengths_host, const int* offsets_host, int S, float* y_cut_dev, float* mu_y_cut_dev,
                        float* y_cut_mask_dev, dex_stream_t s);

/* ---- Griffin-Lim mel inversion (audio/tools.py:18-34 inv_mel_spec -> audio/audio_processing.py:66-82 griffin_lim -> audio/stft.py:52-121
 * STFT.transform / STFT.inverse with window_sumsquare), the reference's only mel -> waveform path without a vocoder checkpoint.  Only
 * the reference configuration: filter_length 1024, hop 256, win_length 1024, periodic Hann, 80 Slaney mels at 22050 Hz.  Every frame
 * is a 1024-point real FFT in LDS (fp32).  Frame counts and lengths are HOST arrays; bad arguments return an error code, with a
 * message in dex_gl_last_error, before anything is enqueued.  No call synchronises or allocates; a row's result does not depend on
 * its batch, and samples past a row's length are 0.  Spectrograms are [B,513,F] (bins x frames, frames contiguous); the waveform of
 * a row of F frames has 256 (F - 1) samples, in rows of 256 (max_frames - 1). */
typedef struct DexGl DexGl;
int  dex_gl_create(DexGl** out);                   /* the handle's tables: FFT twiddles, the window, its square in fp64, the mel basis */
void dex_gl_destroy(DexGl* gl);
const char* dex_gl_last_error(const DexGl* gl);
size_t dex_gl_workspace_bytes(int B, int max_frames);   /* for the inverse and Griffin-Lim; 0 for bad arguments */
/* STFT.transform: wav_dev [B, n_samples], row b lengths_host[b] samples (513 .. n_samples) -> magnitude and atan2 phase
 * [B, 513, n_samples / 256 + 1]; row b fills its first lengths_host[b] / 256 + 1 frames, the rest is not written. */
int  dex_stft_transform(DexGl* gl, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* mag_dev,
                        float* phase_dev, dex_stream_t stream);
/* STFT.inverse: mag, phase [B, 513, max_frames], row b frames_host[b] frames (2 .. max_frames) -> wav_dev [B, 256 (max_frames - 1)]. */
int  dex_stft_inverse(DexGl* gl, const float* mag_dev, const float* phase_dev, const int32_t* frames_host, int B, int max_frames,
                      float* wav_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* griffin_lim with the initial angles given: signal = inverse(S, angles), then n_iters >= 0 times signal = inverse(S, phase(transform
 * (signal))).  mag, angles [B, 513, max_frames], row b frames_host[b] frames (4 .. max_frames) -> wav_dev [B, 256 (max_frames - 1)].
 * 2 (n_iters + 1) launches per 64 rows. */
int  dex_griffin_lim(DexGl* gl, const float* mag_dev, const float* angles_dev, const int32_t* frames_host, int B, int max_frames,
                     int n_iters, float* wav_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* inv_mel_spec's spec_from_mel[:, :, :-1]: mel [B, 80, T] (row b mel_frames_host[b] frames, 2 .. T) -> 1000 exp(mel)^T mel_basis,
 * [B, 513, T - 1]: row b fills mel_frames_host[b] - 1 frames (its last mel frame is dropped) and 0 past them. */
int  dex_mel_to_linear(DexGl* gl, const float* mel_dev, const int32_t* mel_frames_host, int B, int T, float* spec_dev,
                       dex_stream_t stream);

/* ---- Speaker similarity (the reference's src/metric.py:69-95, 115-142, Evaluater.calculate_accept / calculate_asv_score): the d-vector of
 * resemblyzer's VoiceEncoder - 16 kHz, 25 ms window (n_fft 400), hop 160, 40 Slaney mels of the POWER spectrogram (no logarithm),
 * partials of 160 frames, LSTM(40, 256, 3) with gates i | f | g | o, Linear(256, 256), ReLU, L2 normalisation - and the cosine of two
 * of them.  The network is fp32 throughout.  Lengths and the slice table are HOST arrays; bad arguments return an error code, with a
 * message in the handle's last error, before anything is enqueued.  No compute call synchronises or allocates; a row's result does
 * not depend on its batch.  trim_long_silences (webrtcvad) is not part of the library. */
typedef struct DexSpk DexSpk;
#define DEX_SPK_MELS 40
#define DEX_SPK_EMBED 256
#define DEX_SPK_PARTIAL_FRAMES 160
int  dex_spk_create(DexSpk** out);                 /* the handle's tables: DFT twiddles, window and mel basis (fp64) */
void dex_spk_destroy(DexSpk* spk);
const char* dex_spk_last_error(const DexSpk* spk);
/* one weight under resemblyzer's checkpoint key (lstm.weight_ih_l0 [1024,40], lstm.weight_hh_l0 [1024,256], lstm.bias_ih_l0 [1024], ...,
 * linear.weight [256,256], linear.bias [256]); stream-ordered.  The call that loads the last missing key also packs the operands;
 * compute calls return DEX_ERR_STATE until then. */
int  dex_spk_load(DexSpk* spk, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream);
size_t dex_spk_forward_workspace_bytes(int P, int T);      /* P rows of T frames; 0 for bad arguments */
size_t dex_spk_workspace_bytes(int P, int max_samples);    /* the embedding of P partials in all; 0 for bad arguments */
/* wav_to_mel_spectrogram: wav_dev [B, n_samples], row b lengths_host[b] samples (1 .. n_samples) -> mel_dev [B, n_samples / 160 + 1, 40]
 * (frames x channels); row b fills lengths_host[b] / 160 + 1 frames and 0 past them.  center = True with zero padding. */
int  dex_spk_mel(DexSpk* spk, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* mel_dev, dex_stream_t stream);
/* VoiceEncoder.forward: mels_dev [P, T, 40] -> embeds_dev [P, 256] (unit rows), T >= 1. */
int  dex_spk_forward(DexSpk* spk, const float* mels_dev, int P, int T, float* embeds_dev, void* workspace_dev, size_t workspace_bytes,
                     dex_stream_t stream);
/* embed_utterance for a ragged batch: wav_dev [B, n_samples], row b lengths_host[b] samples; utterance b owns slices_host[b] >= 1
 * consecutive entries of slice_start_host (first mel frame of each 160-frame partial, P entries in all; samples past the row's length
 * count as 0, which is the zero padding to the last slice's end).  Mel, slicing, network, the mean over an utterance's partials and its
 * normalisation run in one stream-ordered sequence -> embeds_dev [B, 256]; partials_dev [P, 256] (optional) receives the partial embeddings. */
int  dex_spk_embed(DexSpk* spk, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, const int32_t* slices_host,
                   const int32_t* slice_start_host, int P, float* embeds_dev, float* partials_dev, void* workspace_dev,
                   size_t workspace_bytes, dex_stream_t stream);
/* normalize_volume(wav, target_dBFS, increase_only = True): row b times 10^((target - dBFS_b) / 20) where that is >= 1, unchanged
 * otherwise; dBFS_b = 10 log10(mean(wav_b^2)) with the mean in fp64.  out_dev [B, n_samples] (may be wav_dev), 0 past a row's length. */
int  dex_spk_normalize_volume(DexSpk* spk, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, double target_dbfs,
                              float* out_dev, dex_stream_t stream);
/* calculate_accept: cos_dev [B] = <a_b, b_b> / (|a_b| |b_b|) of rows of a_dev, b_dev [B, D]. */
int  dex_spk_cosine(DexSpk* spk, const float* a_dev, const float* b_dev, int B, int D, float* cos_dev, dex_stream_t stream);

/* ---- ASR score (the reference's src/metric.py:21-67, Evaluater.transcribe / calculate_asr_score): the forward pass of HF's
 * Wav2Vec2ForCTC in eval mode (facebook/wav2vec2-large-960h-lv60-self and its family: layer-norm feature extractor, stable layer
 * norm, head_dim 64) and greedy CTC, in fp32.  Input normalisation (Wav2Vec2FeatureExtractor, do_normalize) is part of the call.
 * Lengths are HOST arrays; bad arguments return an error code, with a message in the handle's last error, before anything is
 * enqueued.  No compute call synchronises or allocates; a row's logits do not depend on its batch.  Edit distance and string work
 * (WER / CER) are the caller's: dex_tts_amd/asr.py. */
typedef struct DexAsr DexAsr;
#define DEX_ASR_MAX_CONV 8
typedef struct {
    int32_t n_conv;                                   /* feature-extractor layers (7) */
    int32_t conv_dim[DEX_ASR_MAX_CONV], conv_kernel[DEX_ASR_MAX_CONV], conv_stride[DEX_ASR_MAX_CONV];
    int32_t conv_bias;                                /* 1: the convolutions carry a bias */
    int32_t feat_extract_norm_layer;                  /* 1 = 'layer' (the only one built) */
    int32_t hidden, n_layers, n_heads, intermediate;
    int32_t do_stable_layer_norm;                     /* 1 (the only one built) */
    int32_t num_conv_pos_embeddings, num_conv_pos_embedding_groups;
    float   layer_norm_eps;
    int32_t vocab;
} DexAsrConfig;
/* NULL = the large-lv60-self values.  DEX_ERR_ARG (and *out = NULL) for a config outside the family that is built. */
int  dex_asr_create(const DexAsrConfig* cfg, DexAsr** out);
void dex_asr_destroy(DexAsr* asr);
const char* dex_asr_last_error(const DexAsr* asr);
/* one weight under its HF state-dict key (wav2vec2.feature_extractor.conv_layers.0.conv.weight ..., lm_head.bias; the positional
 * convolution as ...pos_conv_embed.conv.weight_g [1,1,k] / weight_v [hidden, hidden / groups, k]); stream-ordered */
int  dex_asr_load(DexAsr* asr, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream);
/* packs the operands (weight norm folded in fp64); DEX_ERR_STATE names the first key that was never loaded */
int  dex_asr_finalize(DexAsr* asr, dex_stream_t stream);
int  dex_asr_num_weights(const DexAsr* asr);
int  dex_asr_weight_info(const DexAsr* asr, int i, const char** key, int64_t shape[4], int* ndim);
/* host only: frames of n_samples samples, floor((L - k) / s) + 1 chained over the layers (0 below the receptive field; NULL = default config) */
int  dex_asr_num_frames(const DexAsrConfig* cfg, int n_samples);
size_t dex_asr_workspace_bytes(const DexAsr* asr, int B, int max_samples);     /* 0 for bad arguments */
/* (x - mean) / sqrt(var + 1e-7) per row over its own length, biased variance, statistics in fp64; out_dev [B, n_samples] (may be
 * wav_dev), 0 past a row's length */
int  dex_asr_normalize(DexAsr* asr, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* out_dev, dex_stream_t stream);
/* wav_dev [B, n_samples] raw samples, row b lengths_host[b] samples (every row at least one frame long) -> logits_dev [B, T, vocab],
 * T = dex_asr_num_frames(n_samples); row b fills dex_asr_num_frames(lengths_host[b]) frames and 0 past them */
int  dex_asr_logits(DexAsr* asr, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* logits_dev,
                    void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* dex_asr_logits + dex_asr_ctc with the logits kept in the workspace: ids_dev [B, T] int32, counts_dev [B] int32 */
int  dex_asr_transcribe(DexAsr* asr, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int32_t* ids_dev,
                        int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* greedy CTC: per frame the FIRST index of the maximum (torch.argmax), repeats collapsed, blank (id 0) dropped.  logits_dev [B, T, V],
 * row b frames_host[b] frames (0 .. T) -> ids_dev [B, T] (the first counts_dev[b] entries of a row; the rest 0), counts_dev [B] */
int  dex_asr_ctc(DexAsr* asr, const float* logits_dev, const int32_t* frames_host, int B, int T, int V, int32_t* ids_dev,
                 int32_t* counts_dev, dex_stream_t stream);

/* ---- CTC forced alignment and text likelihood (the contract is the docstring of dex_tts_amd/ctc_align.py; tests/ctc_ref.py restates
 * it in numpy).  logits_dev [B, T, V] fp32, row b frames_host[b] frames; the known text of row b is targets_host[b, 0 .. L_b) of
 * [B, Lmax] int32, L_b = target_lengths_host[b], ids in [0, V) and none equal to blank.  Stateless.  Targets and lengths are HOST
 * arrays, copied to the workspace in stream order and validated first: DEX_ERR_ARG, with nothing enqueued, for a null pointer, an id
 * outside [0, V) or equal to blank, blank outside [0, V), L_b outside [0, Lmax], Lmax outside [0, DEX_CTC_MAX_TARGET], frames outside
 * [1, T], T outside [1, DEX_CTC_MAX_FRAMES], V outside [1, 65536] or B outside [1, DEX_CTC_MAX_ROWS]; DEX_ERR_WORKSPACE below the
 * bytes the sizing call returns.  targets_host may be NULL where Lmax is 0.  Every output of a row is bitwise that of the row alone. */
#define DEX_CTC_MAX_FRAMES 4096
#define DEX_CTC_MAX_TARGET 1023
#define DEX_CTC_MAX_ROWS 1024
size_t dex_ctc_workspace_bytes(int B, int T, int V, int Lmax);          /* 0 for bad arguments */
/* nll_dev [B] fp64: the negative log-likelihood of the text, F.ctc_loss(log_softmax(x), reduction='none'); +inf for a row whose text
 * does not fit its frames */
int  dex_ctc_nll(const float* logits_dev, const int32_t* frames_host, int B, int T, int V, const int32_t* targets_host,
                 const int32_t* target_lengths_host, int Lmax, int blank, double* nll_dev, void* workspace_dev, size_t workspace_bytes,
                 dex_stream_t stream);
/* the Viterbi path over the 2 L + 1 states: states_dev [B, T] int32 (-1 past a row's frames), spans_dev [B, Lmax, 2] int32 (first frame,
 * one past the last frame of each target position; -1 past L_b), token_scores_dev [B, Lmax] fp64 (NaN past L_b), score_dev [B] fp64;
 * nll_dev [B] fp64 is optional (NULL: not computed).  A row whose score is -inf or NaN has no alignment: states and spans -1, token
 * scores NaN. */
int  dex_ctc_align(const float* logits_dev, const int32_t* frames_host, int B, int T, int V, const int32_t* targets_host,
                   const int32_t* target_lengths_host, int Lmax, int blank, int32_t* states_dev, int32_t* spans_dev,
                   double* token_scores_dev, double* score_dev, double* nll_dev, void* workspace_dev, size_t workspace_bytes,
                   dex_stream_t stream);
/* the network's logits, kept in its workspace, followed by the alignment and the likelihood in one stream-ordered sequence; the frames of
 * row b are those of lengths_host[b], T those of n_samples (at most DEX_CTC_MAX_FRAMES).  ctc_workspace_dev holds the bytes the CTC sizing
 * call returns for (B, T, vocab, Lmax); blank is id 0. */
int  dex_asr_align(DexAsr* asr, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, const int32_t* targets_host,
                   const int32_t* target_lengths_host, int Lmax, int32_t* states_dev, int32_t* spans_dev, double* token_scores_dev,
                   double* score_dev, double* nll_dev, void* ctc_workspace_dev, size_t ctc_workspace_bytes, void* workspace_dev,
                   size_t workspace_bytes, dex_stream_t stream);

/* ---- WavLM x-vector speaker similarity (SIM): the embeddings of HF's WavLMForXVector in eval mode with attention_mask = None
 * (microsoft/wavlm-base-plus-sv and its family: group-norm feature extractor, post-layer-norm encoder, head_dim 64, softmax attention
 * with the gated relative-position bias, TDNN / statistics-pooling head), in fp32.  Row b of a batch is the network applied to row b
 * alone at its own length (a zero-padded batch through HF without a mask is not: its group norm sees the padding).  The cosine of two
 * embeddings is dex_spk_cosine.  Lengths are HOST arrays; bad arguments return an error code, with a message in the handle's last
 * error, before anything is enqueued.  No compute call synchronises or allocates; a row's result does not depend on its batch.
 * One call takes rows of at most DEX_WAVLM_MAX_FRAMES encoder frames (81 s at 16 kHz); every row needs at least two frames after the
 * TDNN layers (dex_wavlm_min_samples: the unbiased deviation over one frame is undefined). */
typedef struct DexWavlm DexWavlm;
#define DEX_WAVLM_MAX_CONV 8
#define DEX_WAVLM_MAX_TDNN 8
#define DEX_WAVLM_MAX_FRAMES 4096
typedef struct {
    int32_t n_conv;                                   /* feature-extractor layers (7) */
    int32_t conv_dim[DEX_WAVLM_MAX_CONV], conv_kernel[DEX_WAVLM_MAX_CONV], conv_stride[DEX_WAVLM_MAX_CONV];
    int32_t conv_bias;                                /* 1: the convolutions carry a bias (0 in base-plus-sv) */
    int32_t feat_extract_norm_group;                  /* 1 = 'group' (the only one built) */
    int32_t hidden, n_layers, n_heads, intermediate;
    int32_t do_stable_layer_norm;                     /* 0 (the only one built) */
    int32_t num_conv_pos_embeddings, num_conv_pos_embedding_groups;
    float   layer_norm_eps;
    int32_t num_buckets, max_bucket_distance;         /* relative-position buckets (320, 800) */
    int32_t use_weighted_layer_sum;                   /* 1: softmax(layer_weights)-weighted sum of the n_layers + 1 hidden states */
    int32_t n_tdnn;                                   /* TDNN layers (5) */
    int32_t tdnn_dim[DEX_WAVLM_MAX_TDNN], tdnn_kernel[DEX_WAVLM_MAX_TDNN], tdnn_dilation[DEX_WAVLM_MAX_TDNN];
    int32_t xvector_output_dim;
} DexWavlmConfig;
/* NULL = the base-plus-sv values.  DEX_ERR_ARG (and *out = NULL) for a config outside the family that is built. */
int  dex_wavlm_create(const DexWavlmConfig* cfg, DexWavlm** out);
void dex_wavlm_destroy(DexWavlm* w);
const char* dex_wavlm_last_error(const DexWavlm* w);
/* one weight under its HF state-dict key (wavlm.feature_extractor.conv_layers.0.conv.weight ..., feature_extractor.bias; the positional
 * convolution as ...pos_conv_embed.conv.weight_g [1,1,k] / weight_v [hidden, hidden / groups, k]); stream-ordered */
int  dex_wavlm_load(DexWavlm* w, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream);
/* packs the operands (weight norm folded in fp64, the layer weights' softmax, the bucket table); DEX_ERR_STATE names the first key
 * that was never loaded */
int  dex_wavlm_finalize(DexWavlm* w, dex_stream_t stream);
int  dex_wavlm_num_weights(const DexWavlm* w);
int  dex_wavlm_weight_info(const DexWavlm* w, int i, const char** key, int64_t shape[4], int* ndim);
/* host only (NULL = default config): encoder frames of n_samples samples; the fewest samples a row may have (5200 by default) */
int  dex_wavlm_num_frames(const DexWavlmConfig* cfg, int n_samples);
int  dex_wavlm_min_samples(const DexWavlmConfig* cfg);
/* host only: out[d + n - 1] = _relative_positions_bucket(d) for the key-minus-query distances d = -(n - 1) .. n - 1 */
int  dex_wavlm_rel_buckets(const DexWavlmConfig* cfg, int n, int32_t* out);
size_t dex_wavlm_workspace_bytes(const DexWavlm* w, int B, int max_samples);     /* 0 for bad arguments */
/* wav_dev [B, n_samples] raw samples, row b lengths_host[b] samples; do_normalize != 0: Wav2Vec2FeatureExtractor's normalisation
 * first (dex_asr_normalize) -> hidden_dev [B, T, hidden], T = dex_wavlm_num_frames(n_samples): the layer-mixed hidden states the
 * head reads; row b fills dex_wavlm_num_frames(lengths_host[b]) frames and 0 past them */
int  dex_wavlm_hidden(DexWavlm* w, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize,
                      float* hidden_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* the same inputs -> embed_dev [B, xvector_output_dim]: WavLMForXVector.forward(...).embeddings of every row alone */
int  dex_wavlm_embed(DexWavlm* w, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize,
                     float* embed_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);

/* ---- WavLM-large + ECAPA-TDNN speaker similarity (the SIM-o of zero-shot TTS tables): HF's WavLMModel of the large family
 * (layer-norm feature extractor, stable-layer-norm encoder, head_dim 64, gated relative-position bias; all n_layers + 1 hidden states)
 * feeding the ECAPA-TDNN head of the UniSpeech speaker-verification recipe (softmax(feature_weight) layer mix, InstanceNorm1d, three
 * SE-Res2 blocks, attentive statistics pooling, BatchNorm, Linear), eval mode, fp32.  Written down from a reading of the public
 * code and NOT checked against the real checkpoint.  Row b of a batch is the network applied to row b alone at its own length: every
 * statistic and every convolution's zero padding end at the row's own frames.  The cosine of two embeddings is dex_spk_cosine.
 * Lengths are HOST arrays; bad arguments return an error code, with a message in the handle's last error, before anything is
 * enqueued.  No compute call synchronises or allocates.  One call takes rows of at most DEX_ECAPA_MAX_FRAMES encoder frames; every
 * row needs two (dex_ecapa_min_samples: the instance norm over one frame is undefined). */
typedef struct DexEcapa DexEcapa;
#define DEX_ECAPA_MAX_CONV 8
#define DEX_ECAPA_MAX_FRAMES 4096
#define DEX_ECAPA_BLOCKS 3
#define DEX_ECAPA_RES2_TILE 72                        /* frames one workgroup of the Res2 chain stores */
typedef struct {
    int32_t n_conv;                                   /* feature-extractor layers (7) */
    int32_t conv_dim[DEX_ECAPA_MAX_CONV], conv_kernel[DEX_ECAPA_MAX_CONV], conv_stride[DEX_ECAPA_MAX_CONV];
    int32_t conv_bias;                                /* 1 in wavlm-large */
    int32_t feat_extract_norm_layer;                  /* 1 = 'layer' (the only one built) */
    int32_t hidden, n_layers, n_heads, intermediate;
    int32_t do_stable_layer_norm;                     /* 1 (the only one built) */
    int32_t num_conv_pos_embeddings, num_conv_pos_embedding_groups;
    float   layer_norm_eps;
    int32_t num_buckets, max_bucket_distance;         /* relative-position buckets (320, 800) */
    int32_t channels, emb_dim;                        /* ECAPA_TDNN(channels = 512, emb_dim = 256) */
    int32_t res2_scale;                               /* 8 (the only one built); channels / 8 must be 32 or 64 */
    int32_t se_bottleneck_dim, attention_channels;    /* 128, 128 */
    int32_t global_context_att;                       /* 1: the pooling's attention also reads each channel's mean and deviation over time */
    int32_t dilations[DEX_ECAPA_BLOCKS];              /* of the three SE-Res2 blocks (2, 3, 4), each 1 .. 4 */
} DexEcapaConfig;
/* NULL = the wavlm-large / ECAPA_TDNN(512, 256) values.  DEX_ERR_ARG (and *out = NULL) for a config outside the family that is built. */
int  dex_ecapa_create(const DexEcapaConfig* cfg, DexEcapa** out);
void dex_ecapa_destroy(DexEcapa* e);
const char* dex_ecapa_last_error(const DexEcapa* e);
/* one weight under its key: the trunk's HF keys under wavlm. (the positional convolution as weight_g / weight_v), then the head's
 * UniSpeech names: feature_weight, layer1.{conv,bn}.*, layerN.{Conv1dReluBn1,Conv1dReluBn2}.{conv,bn}.*, layerN.Res2Conv1dReluBn.
 * {convs,bns}.i.*, layerN.SE_Connect.linear{1,2}.*, conv.*, pooling.linear{1,2}.*, bn.*, linear.*; stream-ordered */
int  dex_ecapa_load(DexEcapa* e, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream);
/* packs the operands (weight norm and every eval-mode BatchNorm folded in fp64, the layer weights' softmax, the bucket table) */
int  dex_ecapa_finalize(DexEcapa* e, dex_stream_t stream);
int  dex_ecapa_num_weights(const DexEcapa* e);
int  dex_ecapa_weight_info(const DexEcapa* e, int i, const char** key, int64_t shape[4], int* ndim);
/* host only (NULL = default config): encoder frames of n_samples samples; the fewest samples a row may have (720: two frames) */
int  dex_ecapa_num_frames(const DexEcapaConfig* cfg, int n_samples);
int  dex_ecapa_min_samples(const DexEcapaConfig* cfg);
size_t dex_ecapa_workspace_bytes(const DexEcapa* e, int B, int max_samples);     /* 0 for bad arguments */
/* wav_dev [B, n_samples] raw samples, row b lengths_host[b] samples; do_normalize != 0: (x - mean) / sqrt(var + 1e-5) per row first
 * (the upstream's F.layer_norm(wav, wav.shape)) -> hidden_dev [B, T, hidden], T = dex_ecapa_num_frames(n_samples): the
 * softmax(feature_weight)-mixed hidden states after the head's instance norm; row b fills its own frames and 0 past them */
int  dex_ecapa_hidden(DexEcapa* e, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize,
                      float* hidden_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* the same inputs -> embed_dev [B, emb_dim]: the speaker embedding of every row alone */
int  dex_ecapa_embed(DexEcapa* e, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize,
                     float* embed_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* the Res2 chain of SE-Res2 block `block` (0 .. 2) alone, one launch: x_dev [B, T, channels], row b frames_host[b] frames (1 .. T)
 * -> out_dev [B, T, channels] (not x_dev): seven dilated convolutions with ReLU and BatchNorm over the first seven channel slices,
 * each zero-padded at the row's own ends, the eighth slice copied; 0 past a row's frames */
int  dex_ecapa_res2(DexEcapa* e, int block, const float* x_dev, const int32_t* frames_host, int B, int T, float* out_dev,
                    dex_stream_t stream);

/* ---- UTMOS naturalness score (MOS prediction): the UTMOS22 "strong learner" in eval mode, fp32 - the wav2vec 2.0 base trunk
 * (group-norm feature extractor, post-layer-norm encoder, head_dim 64, plain softmax attention; last_hidden_state), every frame
 * conditioned on a domain and a listener embedding, a bidirectional single-layer LSTM, Linear - ReLU - Linear per frame, and
 * mean over the frames x 2 + 3.  Row b of a batch is the network applied to row b alone at its own length: the group norm, the
 * attention keys, the reverse direction of the LSTM (which starts at the row's own last frame) and the mean end at its own frames.
 * Lengths and ids are HOST arrays; bad arguments return an error code, with a message in the handle's last error, before anything
 * is enqueued.  No compute call synchronises or allocates.  One call takes rows of at most DEX_MOS_MAX_FRAMES encoder frames; every
 * row needs one frame (dex_mos_min_samples). */
typedef struct DexMos DexMos;
#define DEX_MOS_MAX_CONV 8
#define DEX_MOS_MAX_FRAMES 4096
#define DEX_MOS_MAX_LSTM 512
typedef struct {
    int32_t n_conv;                                   /* feature-extractor layers (7) */
    int32_t conv_dim[DEX_MOS_MAX_CONV], conv_kernel[DEX_MOS_MAX_CONV], conv_stride[DEX_MOS_MAX_CONV];
    int32_t conv_bias;                                /* 1: the convolutions carry a bias (0 in wav2vec2-base) */
    int32_t feat_extract_norm_group;                  /* 1 = 'group' (the only one built) */
    int32_t hidden, n_layers, n_heads, intermediate;
    int32_t do_stable_layer_norm;                     /* 0 (the only one built) */
    int32_t num_conv_pos_embeddings, num_conv_pos_embedding_groups;
    float   layer_norm_eps;
    int32_t num_domains, domain_dim, num_judges, judge_dim;    /* Embedding(3, 128), Embedding(3000, 128) */
    int32_t lstm_hidden;                              /* H of the bidirectional LSTM: a multiple of 64 up to DEX_MOS_MAX_LSTM (512) */
    int32_t proj_hidden;                              /* width of the projection's hidden layer (2048) */
} DexMosConfig;
/* NULL = the UTMOS22 strong-learner values.  DEX_ERR_ARG (and *out = NULL) for a config outside the family that is built. */
int  dex_mos_create(const DexMosConfig* cfg, DexMos** out);
void dex_mos_destroy(DexMos* m);
const char* dex_mos_last_error(const DexMos* m);
/* one weight under its key: the trunk's HF keys under wav2vec2. (the positional convolution as weight_g / weight_v),
 * domain_embedding.weight, judge_embedding.weight, decoder_rnn.{weight_ih,weight_hh,bias_ih,bias_hh}_l0[_reverse],
 * projection.0.{weight,bias}, projection.3.{weight,bias}; stream-ordered */
int  dex_mos_load(DexMos* m, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream);
int  dex_mos_finalize(DexMos* m, dex_stream_t stream);
int  dex_mos_num_weights(const DexMos* m);
int  dex_mos_weight_info(const DexMos* m, int i, const char** key, int64_t shape[4], int* ndim);
/* host only (NULL = default config): encoder frames of n_samples samples; the fewest samples a row may have (400: one frame) */
int  dex_mos_num_frames(const DexMosConfig* cfg, int n_samples);
int  dex_mos_min_samples(const DexMosConfig* cfg);
size_t dex_mos_workspace_bytes(const DexMos* m, int B, int max_samples);         /* 0 for bad arguments */
size_t dex_mos_bilstm_workspace_bytes(const DexMos* m, int B, int T);            /* of dex_mos_bilstm; 0 for bad arguments */
/* wav_dev [B, n_samples] raw samples, row b lengths_host[b] samples; do_normalize != 0: zero mean and unit variance per row first
 * -> hidden_dev [B, T, hidden], T = dex_mos_num_frames(n_samples): last_hidden_state; row b fills its own frames and 0 past them */
int  dex_mos_hidden(DexMos* m, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, int do_normalize,
                    float* hidden_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* the recurrence alone: feat_dev [B, T, hidden], row b frames_host[b] frames (1 .. T), conditioned on domain_host[b], judge_host[b]
 * -> out_dev [B, T, 2 x lstm_hidden] (forward | reverse), 0 past a row's frames */
int  dex_mos_bilstm(DexMos* m, const float* feat_dev, const int32_t* frames_host, const int32_t* domain_host, const int32_t* judge_host,
                    int B, int T, float* out_dev, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* the whole network -> frames_dev [B, T]: the projection's score of every frame, 0 past a row's frames */
int  dex_mos_frames(DexMos* m, const float* wav_dev, const int32_t* lengths_host, const int32_t* domain_host, const int32_t* judge_host,
                    int B, int n_samples, int do_normalize, float* frames_dev, void* workspace_dev, size_t workspace_bytes,
                    dex_stream_t stream);
/* the whole network -> score_dev [B]: mean over the row's own frames x 2 + 3 */
int  dex_mos_score(DexMos* m, const float* wav_dev, const int32_t* lengths_host, const int32_t* domain_host, const int32_t* judge_host,
                   int B, int n_samples, int do_normalize, float* score_dev, void* workspace_dev, size_t workspace_bytes,
                   dex_stream_t stream);

/* ---- Whisper ASR score: HF's WhisperForConditionalGeneration in eval mode (log-mel front end of WhisperFeatureExtractor, encoder,
 * decoder with a key/value cache, greedy decoding), in fp32.  The family built: head_dim 64, erf GELU, scale_embedding = False,
 * learned decoder positions, num_mel_bins <= 128.  One workspace carries a batch from dex_whisper_encode (encoder output, the
 * cross-attention keys and values of every decoder layer) through dex_whisper_forward / dex_whisper_generate (the self-attention
 * cache, the decode state), so those calls take the same B and the same workspace.  A row's results do not depend on its batch:
 * every launch fixes its split and summation order from the config and the position.  Bad arguments return an error code, with a
 * message in the handle's last error, before anything is enqueued.  dex_tts_amd/whisper.py states the definitions. */
typedef struct DexWhisper DexWhisper;
#define DEX_WHISPER_MAX_B 32
#define DEX_WHISPER_N_FFT 400
#define DEX_WHISPER_HOP 160
typedef struct {
    int32_t vocab_size, num_mel_bins, d_model;
    int32_t encoder_layers, encoder_attention_heads, encoder_ffn_dim;
    int32_t decoder_layers, decoder_attention_heads, decoder_ffn_dim;
    int32_t max_source_positions, max_target_positions;
    int32_t scale_embedding;                          /* 0 (the only one built) */
    int32_t activation_gelu;                          /* 1 = 'gelu' (the only one built) */
} DexWhisperConfig;
/* NULL = the whisper-large-v3 values.  DEX_ERR_ARG (and *out = NULL) for a config outside the family that is built. */
int  dex_whisper_create(const DexWhisperConfig* cfg, DexWhisper** out);
void dex_whisper_destroy(DexWhisper* w);
const char* dex_whisper_last_error(const DexWhisper* w);
/* one weight under its HF state-dict key (model.encoder.conv1.weight ..., model.decoder.layer_norm.bias); stream-ordered */
int  dex_whisper_load(DexWhisper* w, const char* key, const float* w_dev, const int64_t* shape, int ndim, dex_stream_t stream);
int  dex_whisper_finalize(DexWhisper* w, dex_stream_t stream);
int  dex_whisper_num_weights(const DexWhisper* w);
int  dex_whisper_weight_info(const DexWhisper* w, int i, const char** key, int64_t shape[4], int* ndim);
size_t dex_whisper_workspace_bytes(const DexWhisper* w, int B);                  /* 0 for bad arguments; B <= DEX_WHISPER_MAX_B */
/* host only: the mel filter bank [201][n_mels] in float64 (Slaney scale and norm, 0 - 8000 Hz at 16 kHz) */
int  dex_whisper_mel_filters(int n_mels, double* out);
/* wav_dev [B, n_samples] at 16 kHz, row b lengths_host[b] samples (what lies past them is not read), n_samples <= 2 x
 * max_source_positions x 160 -> out_dev [B, num_mel_bins, 2 x max_source_positions].  Needs no weights. */
int  dex_whisper_log_mel(DexWhisper* w, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* out_dev,
                         void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* feat_dev [B, num_mel_bins, 2 x max_source_positions] -> the encoder output and every decoder layer's cross-attention keys and
 * values, kept in the workspace; enc_out_dev [B, max_source_positions, d_model] (or NULL) receives a copy of the encoder output.
 * ms_host [2] (or NULL; the measuring form, which waits for the stream) receives the milliseconds of the encoder and of the
 * cross-attention projections. */
int  dex_whisper_encode(DexWhisper* w, const float* feat_dev, int B, float* enc_out_dev, float* ms_host, void* workspace_dev,
                        size_t workspace_bytes, dex_stream_t stream);
/* after dex_whisper_encode: ids_dev [B, L] int32 (every id in [0, vocab): the caller's check), fed one position at a time through
 * the cached step -> logits_dev [B, L, vocab] */
int  dex_whisper_forward(DexWhisper* w, const int32_t* ids_dev, int B, int L, float* logits_dev, void* workspace_dev, size_t workspace_bytes,
                         dex_stream_t stream);
/* after dex_whisper_encode: greedy decoding.  prompt_host [n_prompt] feeds positions 0 .. n_prompt - 1 of every row; suppress_dev /
 * begin_dev [vocab] bytes (non-zero = -inf; begin_dev holds at the first new token and includes suppress_dev).  ids_dev [B, max_new]
 * is filled with eos, then with the tokens; lengths_dev [B] = the tokens of a row before its eos.  The loop ends after max_new
 * tokens, when position max_target_positions is reached, or when a read of the finished count (every sync_every steps; 0 = never)
 * finds every row finished; *steps_host = the tokens decoded.  Synchronises the stream before returning. */
int  dex_whisper_generate(DexWhisper* w, const int32_t* prompt_host, int n_prompt, const uint8_t* suppress_dev, const uint8_t* begin_dev,
                          int eos, int B, int max_new, int sync_every, int32_t* ids_dev, int32_t* lengths_dev, int* steps_host,
                          void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* the cached single-query attention alone (head_dim 64): q_dev [B, heads x 64], k_dev / v_dev [B, cap, heads x 64] over keys
 * 0 .. n_keys - 1 -> out_dev [B, heads x 64], scores scaled by 1 / 8.  new_k_dev / new_v_dev [B, heads x 64] (or both NULL) are
 * first appended at position n_keys - 1, as the self-attention of a step does. */
int  dex_whisper_attend(const float* q_dev, float* k_dev, float* v_dev, const float* new_k_dev, const float* new_v_dev, float* out_dev,
                        int B, int heads, int n_keys, int cap, dex_stream_t stream);
/* one linear of the decoder step alone, y_dev [M, N] = x_dev [M, K] x w_dev [K, N] (M <= 32, K and N multiples of 64): form 0 the
 * skinny-M streaming kernel and its consumer (scratch_dev: dex_whisper_step_linear's partials, at least ceil(K / 64) x M x N
 * floats), form 1 launch_igemm - for tests and for the measurement of the two against the weight's bytes */
int  dex_whisper_step_linear(const float* x_dev, const float* w_dev, float* y_dev, float* scratch_dev, size_t scratch_floats, int M, int K,
                             int N, int form, dex_stream_t stream);
/* the greedy step tail alone: logits_dev [B, V], mask_dev [V] bytes (or NULL) -> ids_dev [B * ld_ids] at column `step`: eos for a
 * row whose finished_dev flag is set, else the first index of the maximum of the unmasked logits; emitting eos sets the flag and
 * adds one to *count_dev, any other id adds one to lengths_dev[b] */
int  dex_whisper_pick(const float* logits_dev, int B, int V, const uint8_t* mask_dev, int eos, int32_t* finished_dev, int32_t* lengths_dev,
                      int32_t* count_dev, int32_t* ids_dev, int ld_ids, int step, dex_stream_t stream);
/* ---- long-form scoring: decoding under the timestamp rule over 30 s windows (dex_tts_amd/whisper.py states the definition) */
#define DEX_WHISPER_MAX_LONG_SAMPLES 28800000       /* the cap of a long row: 30 minutes at 16 kHz */
/* the front end of rows of any length up to the cap: wav_dev [B, n_samples], row b lengths_host[b] samples.  A row of at most one
 * chunk has the chunk's frames (the features of dex_whisper_log_mel); a longer row is reflected at its own ends, has lengths_host[b]
 * / 160 frames and is floored at its own maximum over all of them - 8.  frames_host [B] receives the frame counts; out_dev [B,
 * num_mel_bins, max_frames] (max_frames >= the largest count) is 0 behind a row's frames.  scratch_dev holds the fp64 log-spectrum
 * of the call, B x max_frames x num_mel_bins doubles.  Needs no weights. */
int  dex_whisper_log_mel_long(DexWhisper* w, const float* wav_dev, const int32_t* lengths_host, int B, int n_samples, float* out_dev,
                              int max_frames, int32_t* frames_host, void* scratch_dev, size_t scratch_bytes, dex_stream_t stream);
/* feat_dev [rows, num_mel_bins, max_frames] -> out_dev [active, num_mel_bins, 2 x max_source_positions]: window a is frames
 * [seek_host[a], seek_host[a] + n_host[a]) of row row_host[a], followed by 0.0; active <= DEX_WHISPER_MAX_B */
int  dex_whisper_gather_windows(DexWhisper* w, const float* feat_dev, int rows, int max_frames, const int32_t* row_host,
                                const int32_t* seek_host, const int32_t* n_host, int active, float* out_dev, dex_stream_t stream);
/* dex_whisper_generate under the timestamp rule (WhisperTimeStampLogitsProcessor) between the masks and the argmax: timestamps
 * start at no_timestamps_token_id + 1 (at least max_source_positions + 1 of them), max_initial_timestamp_index -1 for none.  The
 * rule's state (a row's last timestamp and new-token count) lives in the workspace; a step needs no host value. */
int  dex_whisper_generate_ts(DexWhisper* w, const int32_t* prompt_host, int n_prompt, const uint8_t* suppress_dev, const uint8_t* begin_dev,
                             int eos, int no_timestamps_token_id, int max_initial_timestamp_index, int B, int max_new, int sync_every,
                             int32_t* ids_dev, int32_t* lengths_dev, int* steps_host, void* workspace_dev, size_t workspace_bytes,
                             dex_stream_t stream);
/* the step tail under the timestamp rule alone, as dex_whisper_pick (step >= 2): n_new_dev [B] a row's new-token count (the rule's
 * step index i; one is added), last_timestamp_dev [B] its last emitted timestamp id or -1 (updated), its last two new ids are read
 * from ids_dev at columns step - 1 and step - 2 where n_new has them */
int  dex_whisper_pick_ts(const float* logits_dev, int B, int V, const uint8_t* mask_dev, int eos, int no_timestamps_token_id,
                         int max_initial_timestamp_index, int32_t* finished_dev, int32_t* lengths_dev, int32_t* count_dev,
                         int32_t* ids_dev, int ld_ids, int step, int32_t* last_timestamp_dev, int32_t* n_new_dev, dex_stream_t stream);
/* ---- decoding under a policy: temperature fallback with the log-prob and no-speech statistics (dex_tts_amd/whisper.py states the
 * definition).  One attempt of B <= `encoded` rows after dex_whisper_encode of `encoded` rows in the same workspace: decode row b reads
 * the cross-attention keys and values of encoded row rows_host[b], so a retry of some rows does not run the encoder again.
 * `timestamps` != 0 decodes under the timestamp rule (the arguments of dex_whisper_generate_ts).  temperature 0 is greedy (the ids of
 * dex_whisper_generate / _generate_ts bit for bit); above 0 the id is the Gumbel-max sample at Philox4x32-10 counter (id >> 2, step,
 * attempt + 16 x seek_host[b], row_keys_host[b]), key `seed`, word id & 3.  sum_logprob_dev [B] (fp64) and n_scored_dev [B]: the sum
 * over a row's new tokens (its eos included) of the fp64 log-softmax of the masked logits at the token, and their count.
 * no_speech_prob_dev [B] (fp64, or NULL): the softmax of the unprocessed logits at prompt position 0 at no_speech_token_id. */
int  dex_whisper_generate_policy(DexWhisper* w, const int32_t* prompt_host, int n_prompt, const uint8_t* suppress_dev, const uint8_t* begin_dev,
                                 int eos, int timestamps, int no_timestamps_token_id, int max_initial_timestamp_index, double temperature,
                                 uint64_t seed, int attempt, const uint32_t* row_keys_host, const int32_t* seek_host, int encoded,
                                 const int32_t* rows_host, int B, int max_new, int sync_every, int32_t* ids_dev, int32_t* lengths_dev,
                                 double* sum_logprob_dev, int32_t* n_scored_dev, int no_speech_token_id, double* no_speech_prob_dev,
                                 int* steps_host, void* workspace_dev, size_t workspace_bytes, dex_stream_t stream);
/* the policy step tail alone, as dex_whisper_pick (timestamps == 0) or dex_whisper_pick_ts (timestamps != 0, step >= 2) with B <=
 * DEX_WHISPER_MAX_B: `step` is the counter's step word; the chosen id's log-probability is added to sum_logprob_dev[b] and one to
 * n_scored_dev[b] unless the row's finished flag was set */
int  dex_whisper_pick_policy(const float* logits_dev, int B, int V, const uint8_t* mask_dev, int eos, int timestamps, int no_timestamps_token_id,
                             int max_initial_timestamp_index, double temperature, uint64_t seed, int attempt, const uint32_t* row_keys_host,
                             const int32_t* seek_host, int32_t* finished_dev, int32_t* lengths_dev, int32_t* count_dev, int32_t* ids_dev,
                             int ld_ids, int step, int32_t* last_timestamp_dev, int32_t* n_new_dev, double* sum_logprob_dev,
                             int32_t* n_scored_dev, dex_stream_t stream);
/* ---- beam search (dex_tts_amd/whisper.py states the definition): U utterances of K beams are the U x K rows u K + r of a step */
#define DEX_WHISPER_MIN_BEAMS 2
#define DEX_WHISPER_MAX_BEAMS 8
#define DEX_WHISPER_BEAM_KEYS 13000     /* K x keys of one cross-form launch: their scores sit in LDS */
/* The state of U utterances between two tail launches, all on the device.  A row's token sequence and ancestry are read from the
 * _in buffers and written to the _out buffers (the caller swaps them between steps; no element is permuted in place).  Ancestry
 * entries are beam indices 0 .. K - 1 within the utterance.  The pool of finished hypotheses lives in K slots per utterance;
 * pool_order lists an utterance's slots best first, pool_n of them. */
typedef struct DexWhisperBeamState {
    double*  run_score;                 /* [U K] accumulated score of each running beam */
    double*  pool_score;                /* [U K] by slot */
    int32_t* seq_in;  int32_t* seq_out; /* [U K, ld_seq] the new tokens of each running beam */
    int32_t* anc_in;  int32_t* anc_out; /* [U K, ld_anc] the row whose cache slot holds position t of a beam's prefix */
    int32_t* pool_ids;                  /* [U K, ld_seq] by slot */
    int32_t* pool_len;                  /* [U K] by slot: the tokens before the eos; the full count of a capped hypothesis */
    int32_t* pool_order;                /* [U K] */
    int32_t* pool_n;                    /* [U] */
    int32_t* done;                      /* [U] */
    int32_t* count;                     /* [1] the done utterances */
    int32_t  ld_seq, ld_anc;
} DexWhisperBeamState;
/* the single-query attention of K beams per utterance alone (head_dim 64), a row bitwise dex_whisper_attend of that query.
 * anc_dev NULL, the cross form: q_dev [U K, heads x 64] against the utterance's k_dev / v_dev [U, cap, heads x 64] over keys
 * 0 .. n_keys - 1 (K x n_keys <= DEX_WHISPER_BEAM_KEYS), one workgroup per (head, utterance) streaming the keys once.
 * anc_dev [U K, ld_anc] given, the self form: k_dev / v_dev [U K, cap, heads x 64]; row r first appends new_k_dev / new_v_dev
 * [U K, heads x 64] (or both NULL) at position n_keys - 1 of its own row, and reads position t < n_keys - 1 (t <= n_keys - 1 with
 * nothing appended) from row anc[r][t] of its utterance. */
int  dex_whisper_attend_beam(const float* q_dev, float* k_dev, float* v_dev, const float* new_k_dev, const float* new_v_dev,
                             const int32_t* anc_dev, int ld_anc, float* out_dev, int U, int K, int heads, int n_keys, int cap,
                             dex_stream_t stream);
/* the beam step tail alone (its three launches), new-token step `step` at cache position `pos`: logits_dev [U K, V] fp32, mask_dev
 * [V] bytes (or NULL); scratch_dev (8-byte aligned, dex_whisper_beam_pick_scratch_bytes) holds the chunk sums and candidates.
 * `last` marks the last step (every candidate finished).  tokens_dev / parents_dev [U K] (or NULL) receive the new running set of
 * the utterances that were not done (nothing is written on the last step). */
int  dex_whisper_beam_pick(const float* logits_dev, int U, int K, int V, const uint8_t* mask_dev, int eos, int step, int pos, int last,
                           double length_penalty, const DexWhisperBeamState* state, int32_t* tokens_dev, int32_t* parents_dev,
                           void* scratch_dev, size_t scratch_bytes, dex_stream_t stream);
size_t dex_whisper_beam_pick_scratch_bytes(int U, int K, int V);                 /* 0 for bad arguments */
size_t dex_whisper_beam_workspace_bytes(const DexWhisper* w, int U, int K);     /* 0 for bad arguments; U x K <= DEX_WHISPER_MAX_B */
/* Beam search over the cached step after dex_whisper_encode of the U utterances in the same workspace (the encoder's layout of U
 * rows heads it).  ids_dev [U, max_new] (eos behind the hypothesis), lengths_dev [U], scores_dev [U] (fp64).  trace_*_dev (all or
 * none): the fp32 logits [max_new, U K, V], and tokens, parents (int32, -1 where an utterance was done) and running scores (fp64)
 * [max_new, U K] of every step.  pool_*_dev (or NULL): the pool at the end, best first: ids [U K, max_new], lengths and scores
 * [U K], entries [U]. */
int  dex_whisper_generate_beam(DexWhisper* w, const int32_t* prompt_host, int n_prompt, const uint8_t* suppress_dev, const uint8_t* begin_dev,
                               int eos, int U, int K, double length_penalty, int max_new, int sync_every, int32_t* ids_dev,
                               int32_t* lengths_dev, double* scores_dev, int* steps_host, float* trace_logits_dev, int32_t* trace_tokens_dev,
                               int32_t* trace_parents_dev, double* trace_scores_dev, int32_t* pool_ids_dev, int32_t* pool_len_dev,
                               double* pool_scores_dev, int32_t* pool_n_dev, void* workspace_dev, size_t workspace_bytes,
                               dex_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEX_AMD_H */

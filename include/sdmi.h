/* libsdmi -- MI355X (gfx950) native UNet eps-prediction + PLMS/DDIM step for Stable Diffusion v1.
 *
 * C ABI of the drop-in boundary.  The reference (CompVis/stable-diffusion) is pure Python and has no FFI
 * of its own; each entry point below names the reference call it stands in for (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes binding and the yaml `target:` switch that plugs it in.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; sdmi_last_error() gives the thread-local message.
 *   - all pointers are DEVICE pointers on the current HIP device unless stated otherwise;
 *     activations cross the boundary as contiguous fp32 in the reference's own layouts (NCHW latents,
 *     [B,L,D] context, int64 timesteps).
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); the library only enqueues
 *     work on it and never synchronises the device.
 *   - the library owns packed weights; the caller owns inputs, outputs and the workspace.
 */
#ifndef SDMI_H_
#define SDMI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDMI_ABI_VERSION 17

typedef struct sdmi_unet sdmi_unet;

/* Constructor arguments of UNetModel used by configs/stable-diffusion/v1-inference.yaml:29-44
 * (ldm/modules/diffusionmodules/openaimodel.py:443-470).  use_spatial_transformer=True, legacy=False. */
typedef struct sdmi_unet_cfg {
  int32_t in_channels;
  int32_t out_channels;
  int32_t model_channels;
  int32_t num_res_blocks;
  int32_t n_levels;
  int32_t channel_mult[8];
  int32_t n_attention_resolutions;
  int32_t attention_resolutions[8];
  int32_t num_heads;
  int32_t transformer_depth;
  int32_t context_dim;
} sdmi_unet_cfg;

const char* sdmi_last_error(void);
int sdmi_abi_version(void);
/* Always 0: no experiments build exists any more (the kernels that lost their same-box A/Bs were removed).  Kept for callers that ask. */
int sdmi_has_experiments(void);

/* ---- UNet handle: replaces instantiate_from_config(unet_config) + load_state_dict ----------------------- */
/* UNetModel.__init__, openaimodel.py:443-692 */
int sdmi_unet_create(const sdmi_unet_cfg* cfg, sdmi_unet** out);
/* Arithmetic of a UNet handle, fixed when it is created.
 *   MIXED  fp16 MFMA operands, with 3-pass split-fp16 on the op classes the precision allocation names
 *   FULL   every MFMA operand split-fp16 (hi = fp16(x), lo = fp16(x - hi); a_hi b_hi + a_lo b_hi + a_hi b_lo, fp32 accumulation):
 *          3x3 / 1x1 convolutions, resamplers, every linear and both attention products.  The row-strip chains and the
 *          LayerNorm / GroupNorm folds are not used in this mode.  Its packed weights differ: a blob is imported only by a handle of
 *          the mode that wrote it.
 * sdmi_unet_create(cfg, out) = sdmi_unet_create_with_precision(cfg, SDMI_PRECISION_MIXED, out). */
#define SDMI_PRECISION_MIXED 0
#define SDMI_PRECISION_FULL 1
int sdmi_unet_create_with_precision(const sdmi_unet_cfg* cfg, int precision, sdmi_unet** out);
int sdmi_unet_precision(const sdmi_unet* h);      /* SDMI_PRECISION_*, or -1 for a null handle */
/* UNet families beyond SD v1 (additive; sdmi_unet_cfg is unchanged).  The latent-inpainting model
 * (models/ldm/inpainting_big/config.yaml): attention_block = 1, resblock_updown = 1, context_dim = 0.
 *   attention_block  0: SpatialTransformer with cross-attention (use_spatial_transformer=True, legacy=False: SD v1);
 *                    1: the legacy AttentionBlock (openaimodel.py:278-323; use_spatial_transformer=False, legacy=True,
 *                       num_head_channels=-1): GroupNorm -> conv1d qkv -> QKVAttentionLegacy over all pixels -> proj_out, + x.
 *                       No context: sdmi_unet_forward takes ctx = NULL and Lctx = 0; transformer_depth is not read.
 *   resblock_updown  0: Downsample / Upsample convolutions between the levels; 1: ResBlocks with down / up resampling
 *                    (openaimodel.py:208-216,253-259: 2x2 average pool / nearest x2 of GroupNorm+SiLU(x) and of the skip x);
 *                    the latent H and W must then be multiples of 2^(n_levels-1) (avg_pool2d rounds down).
 * sdmi_unet_create_with_precision(cfg, p, out) = sdmi_unet_create_ext(cfg, NULL, p, out) (NULL = all zero). */
typedef struct sdmi_unet_ext {
  int32_t attention_block;
  int32_t resblock_updown;
} sdmi_unet_ext;
int sdmi_unet_create_ext(const sdmi_unet_cfg* cfg, const sdmi_unet_ext* ext, int precision, sdmi_unet** out);
/* ... with a word of creation flags (additive; sdmi_unet_ext is unchanged).  sdmi_unet_create_ext(cfg, ext, p, out) = flags 0.
 *   SDMI_UNET_SCALE_SHIFT_NORM  every ResBlock is a use_scale_shift_norm one (openaimodel.py:267-271): emb_layers.1 is [2 cout][4 mc] and
 *                               h = out_norm(h) * (1 + scale) + shift in front of SiLU and the second convolution, instead of h + emb_out behind
 *                               the first.  The unconditional models (models/ldm/lsun_churches256/config.yaml): needs attention_block = 1 and
 *                               resblock_updown = 1. */
#define SDMI_UNET_SCALE_SHIFT_NORM 1u
/*   SDMI_UNET_NUM_HEAD_CHANNELS(n)  num_head_channels = n (openaimodel.py:532-535,561-563; cfg.num_heads is then not read, pass -1 as the
 *                               reference does): every AttentionBlock runs ch / n heads of n channels, QKVAttentionLegacy row order.  n must divide
 *                               every attention level's channel count and be an instantiated head dim.  attention_block = 1 only.  The face /
 *                               bedroom LDMs (models/ldm/celeba256, ffhq256, lsun_beds256: model_channels 224, n = 32 -> 14 / 21 / 28 heads) and
 *                               bsr_sr (160, n = 32 -> 20 heads).  A handle with attention_block = 1 takes model_channels % 32 == 0 (GEMM sources
 *                               of 32 (mod 64) channels end in a half k-tile); SpatialTransformer handles keep model_channels % 64 == 0.
 *                               A packed blob records n and is imported only by a handle created with the same n.
 *                               Also with attention_block = 0 (additive: a flag value that was refused before, no struct or call changes,
 *                               SDMI_ABI_VERSION stays as it is): every SpatialTransformer runs ch / n heads of n channels
 *                               (openaimodel.py:542-549; legacy True or False give the same heads wherever n divides ch).  Only n = 32 is admitted
 *                               there (the head dim this family is tested at; any other value is refused by name), cfg.num_heads must be -1 and
 *                               n must divide every attention level.  The retrieval-augmented model
 *                               (configs/retrieval-augmented-diffusion/768x768.yaml: model_channels 448, n = 32 -> 14 / 28 / 42 / 56 heads, 16
 *                               latent channels in and out) and layout-to-image (models/ldm/layout2img-openimages256: 128, n = 32). */
#define SDMI_UNET_NUM_HEAD_CHANNELS_SHIFT 16
#define SDMI_UNET_NUM_HEAD_CHANNELS_MASK 0x0fff0000u
#define SDMI_UNET_NUM_HEAD_CHANNELS(n) (((unsigned)(n) << SDMI_UNET_NUM_HEAD_CHANNELS_SHIFT) & SDMI_UNET_NUM_HEAD_CHANNELS_MASK)
int sdmi_unet_create_flags(const sdmi_unet_cfg* cfg, const sdmi_unet_ext* ext, unsigned flags, int precision, sdmi_unet** out);
int sdmi_unet_destroy(sdmi_unet* h);
/* enumerate the state_dict keys the handle expects (= UNetModel.state_dict().keys()) */
int sdmi_unet_num_weights(const sdmi_unet* h);
int sdmi_unet_weight_info(const sdmi_unet* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim);
/* model.load_state_dict (scripts/txt2img.py:56): fp32 tensor in the reference layout (conv OIHW, linear [out,in]);
 * `ptr` may be a device or a host pointer.  The library repacks (fp16 [N][K], K ordered (64-channel chunk, ky, kx, channel)) and keeps its own copy. */
int sdmi_unet_set_weight(sdmi_unet* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream);
/* fails (listing the first missing key) unless every expected tensor was set */
int sdmi_unet_finalize(sdmi_unet* h);

/* Packed-weight blob: the packed device buffers of a finalized handle, behind a header that pins the
 * configuration and ABI version.  `import` replaces every set_weight call + finalize (no fp32 checkpoint, no repack);
 * the buffers are host memory (e.g. an mmap of the file tools/pack_checkpoint.py writes). */
int64_t sdmi_unet_packed_bytes(sdmi_unet* h);
int sdmi_unet_export_packed(sdmi_unet* h, void* host_buf, int64_t bytes, void* stream);
int sdmi_unet_import_packed(sdmi_unet* h, const void* host_buf, int64_t bytes, void* stream);

/* bytes of scratch `sdmi_unet_forward` needs for this shape (0 on error) */
int64_t sdmi_unet_workspace_bytes(sdmi_unet* h, int B, int H, int W, int Lctx);

/* Cross-attention K/V of all SpatialTransformers depend only on the context (attention.py:174-176):
 * compute them once per prompt.  ctx: fp32 [B, Lctx, context_dim]. */
int sdmi_unet_cache_context(sdmi_unet* h, const float* ctx, int B, int Lctx, void* workspace, int64_t workspace_bytes,
                            void* stream);
/* The K / V^T caches are handle-owned device buffers of a fixed capacity: sdmi_unet_finalize reserves room for 8 rows x 77
 * context tokens (the SD-v1 prompt length at the largest batch one call takes).  sdmi_unet_forward NEVER allocates: a
 * context beyond the capacity fails with a message naming this call.  `reserve_context` grows the capacity (grow-only,
 * allocates: call it outside the sampling loop); sdmi_unet_cache_context grows it itself when needed. */
int sdmi_unet_reserve_context(sdmi_unet* h, int B, int Lctx);

/* The timestep path of UNetModel.forward -- timestep_embedding -> time_embed (openaimodel.py:723-724) -> every ResBlock's
 * emb_layers (openaimodel.py:218-224, 22 Linear layers = a 20160 x 1280 fp32 matrix for SD v1) -- depends on the timestep
 * only.  A sampler knows its timesteps in advance (plms.py:121-128, ddim.py:129-134): `cache_timesteps` computes the rows for
 * a list of INTEGER timesteps in one batch (the weights are read once per 8 timesteps instead of once per UNet call; same
 * kernels, rows are independent: bit-identical values), on `stream`, replacing any earlier table.  `hint_timestep(t)`
 * tells the NEXT sdmi_unet_forward that every row of its timestep tensor equals t: if t is in the table the call takes
 * the cached rows and launches nothing for the timestep path; otherwise (or without a hint) it computes them from its
 * timestep tensor as before.  The hint is the caller's assertion -- it is not checked against the device tensor -- and is
 * consumed by that one call.  t_host: host memory.  Setting weights drops the table. */
int sdmi_unet_cache_timesteps(sdmi_unet* h, const int64_t* t_host, int n, void* stream);
int sdmi_unet_hint_timestep(sdmi_unet* h, int64_t t);
/* Launch tapes (ABI 17; csrc/tape.h): sdmi_unet_forward records the launch list of a (B, H, W, Lctx, workspace, timestep mode, knobs) once and
 * replays it -- no dry pass, no table lookups, no descriptor fills -- patching only the caller's pointers (x, eps_out, timesteps, context, the
 * timestep-table row), at the argument words the executor declared for each of them while recording.  There is nothing to call: this
 * reports how many forwards were replayed / recorded (tests, bench.py).  SDMI_REPLAY=0 turns the tapes off; SDMI_REPLAY_VERIFY=1 runs the
 * executor on every would-be replay and fails if the patched tape differs from it.
 * No counterpart in the reference (pure Python, scripts/txt2img.py drives torch ops one by one). */
int sdmi_unet_tape_stats(sdmi_unet* h, int64_t* replayed, int64_t* recorded);
/* Which ResBlocks run their skip_connection as the 1x1 tail phase of conv2's launch (SDMI_SKIP_FOLD, default on) at this
 * shape: a dry pass (host only, like sdmi_unet_workspace_bytes) writes 1 (folded) or 0 per ResBlock with a skip convolution, in execution
 * order, into folded[0 .. cap) and returns their number, or -1. */
int sdmi_unet_skip_fold_plan(sdmi_unet* h, int B, int H, int W, int Lctx, int32_t* folded, int cap);

/* UNetModel.forward(x, timesteps, context) openaimodel.py:710-742, reached through
 * LatentDiffusion.apply_model ddpm.py:891-900,986-992 and DiffusionWrapper.forward ddpm.py:1402-1410.
 *   x        fp32 [B, in_channels, H, W] (NCHW, contiguous)
 *   t_i64 / t_f32   exactly one non-NULL: [B] timesteps (int64 as the samplers pass; fp32 for DPM-Solver)
 *   ctx      fp32 [B, Lctx, context_dim], or NULL to reuse sdmi_unet_cache_context()'s result
 *   eps_out  fp32 [B, out_channels, H, W] -- written fresh on every call; may be x itself (in place), and the other caller buffers
 *            may overlap one another -- a replayed call behaves the same, whatever the buffers of the recorded call were.  None of them
 *            may lie inside the workspace. */
int sdmi_unet_forward(sdmi_unet* h, const float* x, const int64_t* t_i64, const float* t_f32, const float* ctx,
                      float* eps_out, int B, int H, int W, int Lctx, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* ---- sampler step: classifier-free guidance combine + PLMS / DDIM update in one launch -------------------
 * PLMSSampler.p_sample_plms plms.py:172-236, DDIMSampler.p_sample_ddim ddim.py:165-204.
 *   eps_model: model output; cfg != 0 -> rows [0,n) are the unconditional half, [n,2n) the conditional half
 *   mode: 0 e'=e_t | 1 (3e-o0)/2 | 2 (23e-16o0+5o1)/12 | 3 (55e-59o0+37o1-9o2)/24 | 4 (o0+e_t)/2
 *   a_t, a_prev, sigma, sqrt_1m_at: the four table entries the reference indexes per step
 *   noise (optional, sigma>0), e_t_out (optional: post-CFG eps for the history), pred_x0 (optional) */
int sdmi_sampler_step(const float* eps_model, int cfg, float scale, const float* x, int mode, const float* old0,
                      const float* old1, const float* old2, float a_t, float a_prev, float sigma, float sqrt_1m_at,
                      const float* noise, float* e_t_out, float* x_prev, float* pred_x0, int64_t n, void* stream);

/* The same step split at pred_x0, for quantize_x0 (ddim.py:195-197, plms.py:207-209: first_stage_model.quantize(pred_x0) sits between
 * pred_x0 and x_prev).  sdmi_sampler_step_x0 is the first half: the CFG combine, the multistep e' and pred_x0 = (x - sqrt_1m_at e') /
 * sqrt(a_t), the bits sdmi_sampler_step writes; ep_out (required) receives e', e_t_out is optional.  sdmi_sampler_step_from_x0 is the
 * second half from a given pred_x0: x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma^2) ep + sigma noise (noise optional, sigma > 0).
 * The two chained with nothing in between write the x_prev of sdmi_sampler_step. */
int sdmi_sampler_step_x0(const float* eps_model, int cfg, float scale, const float* x, int mode, const float* old0, const float* old1,
                         const float* old2, float a_t, float sqrt_1m_at, float* e_t_out, float* ep_out, float* pred_x0, int64_t n,
                         void* stream);
int sdmi_sampler_step_from_x0(const float* pred_x0, const float* ep, float a_prev, float sigma, const float* noise, float* x_prev,
                              int64_t n, void* stream);

/* ---- the same step for rows at different steps of different schedules: one launch for up to SDMI_SAMPLER_MAX_SLOTS latents -----------
 * What lets requests that arrive one after another share a UNet call (SamplerPoolHIP): each slot is one latent of n elements with its
 * own table entries, history and destinations.  Per slot the arithmetic is sdmi_sampler_step's, op for op, and the host scalars come
 * from the same code: e_t_out, pred_x0 and x_prev are the bits of a lone sdmi_sampler_step call with the slot's arguments.
 *   eps_u, eps_c     two rows of the UNet output; cfg == 0: eps_u alone is read
 *   x, old0..old2, noise, scale, mode, a_t, a_prev, sigma, sqrt_1m_at: as sdmi_sampler_step
 *   outputs, each optional (at least one): e_t_out; x_state_out (x_prev; may be x itself); pred_x0; unet_dst0 / unet_dst1 (the same
 *     x_prev, written where the NEXT UNet call reads this slot's row(s): a guided slot feeds an unconditional and a conditional row);
 *     t_dst0 / t_dst1 receive t_next, the slot's entry in the next call's int64 timestep tensor
 * A slot whose pointers are all 16-byte aligned, with n % 4 == 0, is moved 16 bytes per lane, any other one element by element.
 * The first PLMS step is two slot operations, one per UNet call: mode 0 writing e_t_out and unet_dst* only, then mode 4 with old0 = that
 * e_t.  Additive: no existing struct or call changes, SDMI_ABI_VERSION stays as it is.
 * Refused before anything is launched: n_slots > SDMI_SAMPLER_MAX_SLOTS, n <= 0, a missing pointer, a mode outside 0..4, missing history. */
#define SDMI_SAMPLER_MAX_SLOTS 8
typedef struct sdmi_sampler_slot {
  const float* eps_u; const float* eps_c; const float* x;
  const float* old0; const float* old1; const float* old2;
  const float* noise;
  float* e_t_out; float* x_state_out; float* pred_x0;
  float* unet_dst0; float* unet_dst1;
  int64_t* t_dst0; int64_t* t_dst1;
  int64_t t_next;
  int32_t cfg; int32_t mode;
  float scale; float a_t; float a_prev; float sigma; float sqrt_1m_at;
  int32_t reserved;                 /* 0 */
} sdmi_sampler_slot;                /* 152 bytes */
int sdmi_sampler_step_rows(const sdmi_sampler_slot* slots, int n_slots, int64_t n, void* stream);

/* ---- one launch for up to SDMI_SAMPLER_MAX_SLOTS latents of two kinds: that step, or one evaluation of a DPM-Solver plan -----------------
 * What lets DPM-Solver requests share UNet calls with one another and with PLMS / DDIM requests (SamplerPoolHIP(timesteps='float32')):
 * the next call's timestep tensor is fp32 -- sdmi_unet_forward embeds (float)t_i64[b] or t_f32[b], the same bits for an integer t.
 *   kind 0   the PLMS / DDIM step: eps_u, eps_c, cfg, scale, x, mode, old0..old2, noise, a_t, a_prev, sigma, sqrt_1m_at, e_t_out, pred_x0,
 *            x_state_out, unet_dst0 / 1 exactly as in sdmi_sampler_slot, the same arithmetic from the same code: the bits of
 *            sdmi_sampler_step_rows with these fields.  The fields of kind 1 are ignored.
 *   kind 1   one model evaluation of a DPMPlan and the update that follows it (sdmi_dpm_model_value, then sdmi_dpm_update):
 *            e = eps_u, or with cfg eps_u + scale (eps_c - eps_u);  m = e, or with data_prediction (x - sigma_t e) / alpha_t, x being the
 *            latent the model was evaluated at;  m_out (optional) receives m.
 *            form 0..3: the update of that form over x_base, m0, m1, m2 and c9[9], as sdmi_dpm_update defines them; m_self is a mask of
 *            the operands that ARE the m just computed (bit j: m_j) -- they come from registers and their pointers are not read.
 *            form -1: no update (the last evaluation of denoise_to_zero); the slot's result is m.
 *            x_state_out (may be x_base or x) and unet_dst0 / 1 receive the result.  The fields of kind 0 are ignored.
 *   both     tf_dst0 / tf_dst1 receive t_next, the slot's entry in the next call's fp32 timestep tensor: a kind 0 slot's integer timestep
 *            as float (exact below 2^24), a kind 1 slot's next model-input time.  At least one output other than tf_dst* is required.
 * Every input of a slot is read before its first output is written.  A slot whose pointers are all 16-byte aligned, with n % 4 == 0, is
 * moved 16 bytes per lane, any other one element by element.  There is no thresholding inside a slot: its per-sample quantile sits
 * between the model value and the update.  Additive: no existing struct or call changes, SDMI_ABI_VERSION stays as it is.
 * Refused before anything is launched: n_slots > SDMI_SAMPLER_MAX_SLOTS, n <= 0, a kind other than 0 / 1, a missing pointer the kind /
 * form needs, a mode outside 0..4, missing history, a form outside -1..3, an m_self bit on an operand the form does not read. */
typedef struct sdmi_sampler_plan_slot {
  const float* eps_u; const float* eps_c; const float* x;
  const float* old0; const float* old1; const float* old2; const float* noise;     /* kind 0 */
  const float* x_base; const float* m0; const float* m1; const float* m2;           /* kind 1 */
  float* e_t_out; float* pred_x0;                                                   /* kind 0 */
  float* m_out;                                                                     /* kind 1 */
  float* x_state_out; float* unet_dst0; float* unet_dst1;
  float* tf_dst0; float* tf_dst1;
  int32_t kind; int32_t cfg;
  int32_t mode;                                                                     /* kind 0 */
  int32_t form; int32_t m_self; int32_t data_prediction;                            /* kind 1 */
  float scale; float t_next;
  float a_t; float a_prev; float sigma; float sqrt_1m_at;                           /* kind 0 */
  float alpha_t; float sigma_t; float c9[9];                                        /* kind 1 */
  int32_t reserved;                 /* 0 */
} sdmi_sampler_plan_slot;           /* 248 bytes */
int sdmi_sampler_plan_rows(const sdmi_sampler_plan_slot* slots, int n_slots, int64_t n, void* stream);

/* ---- ancestral DDPM step: LatentDiffusion.p_mean_variance + p_sample (ddpm.py:1047-1107) and the mask blend of p_sample_loop /
 * progressive_denoising (:1203-1205, :1154-1157) in one launch; fp32, each op rounded on its own in the reference's order:
 *   x0 = c_recip x - c_recipm1 eps;  clip != 0: x0 = clamp(x0, -1, 1) (a NaN stays NaN);  mean = coef1 x0 + coef2 x;
 *   x_prev = mean + s noise;  with mask: x_prev = (sa x0_orig + s1ma q_noise) mask + (1 - mask) x_prev
 *   c_recip, c_recipm1, coef1, coef2, sa, s1ma: sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t], posterior_mean_coef1[t],
 *     posterior_mean_coef2[t], sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t] of DDPM.register_schedule
 *   s = (t != 0) * exp(0.5 * posterior_log_variance_clipped[t]);  noise: required with x_prev, already times the temperature
 *   mask (optional; of the latent's full shape), x0_orig, q_noise: the inpainting blend
 *   x0_out (optional) receives x0; x_prev may be x (in place)
 * Two partial forms, for quantize_denoised (the codebook quantizer sits between x0 and the posterior mean):
 *   x_prev NULL: up to x0_out only;   eps NULL and x0_in set: from the given x0 (no clamp). */
int sdmi_ddpm_step(const float* eps, const float* x0_in, const float* x, float c_recip, float c_recipm1, int clip, float coef1,
                   float coef2, float s, const float* noise, const float* mask, const float* x0_orig, const float* q_noise, float sa,
                   float s1ma, float* x0_out, float* x_prev, int64_t n, void* stream);


/* DPM-Solver++ (2M) step as `scripts/txt2img.py --dpm_solver` runs it: classifier-free combine
 * (dpm_solver.py:340-346), data prediction m0 = (x - sigma_s e) / alpha_s (:386-399) and the multistep update
 * order 1: x_next = cx x - a m0 (:519-530);  order 2: x_next = cx x - a m0 - 0.5 a inv_r0 (m0 - m_prev) (:776-790).
 * m_out (optional) receives m0; x_next may be NULL (model value only). */
int sdmi_dpm_solver_step(const float* eps_model, int cfg, float scale, const float* x, const float* m_prev, float alpha_s,
                         float sigma_s, float cx, float a, float inv_r0, int order, float* m_out, float* x_next, int64_t n,
                         void* stream);

/* ---- the other DPM-Solver variants (dpm_solver.py: singlestep, order 3, adaptive, thresholding).  fp32, every op rounded on its own
 * in the reference's order; scalars come from the host, evaluated with the reference's own fp32 ops; -(c v) is passed as (-c) v.
 *
 * Model value (:340-346, :386-408): e = classifier-free combine of eps_model (rows [0,n) uncond, [n,2n) cond when cfg);
 *   predict_x0 == 0: out = e;   else out = (x - sigma_s e) / alpha_s, and with s (device, one per sample of `row` elements):
 *   out = clamp(out, -s[b], s[b]) / s[b] (:397-398). */
int sdmi_dpm_model_value(const float* eps_model, int cfg, float scale, const float* x, int predict_x0, float alpha_s, float sigma_s,
                         const float* s, int64_t row, float* out, int64_t n, void* stream);

/* One update of the reference per launch; c9: nine host floats.
 *   form 0: out = c0 x + c1 m0                                  dpm_solver_first_update (:530-545), x_s1 (:588-591, :682-685)
 *   form 1: out = (c0 x + c1 m0) + c2 (c3 (m1 - m2))            singlestep second update and x_s2, singlestep third 'dpm_solver'
 *                                                               (:594-627, :687-698, :726-737; c3 = 1), multistep second (:783-809; c3 = 1 / r0)
 *   form 2: singlestep third 'taylor' (:700-709, :739-748): D1_0 = c4 (m1 - m0), D1_1 = c5 (m2 - m0), D1 = (c6 D1_0 - c7 D1_1) / c8,
 *           D2 = (2 (D1_1 - D1_0)) / c8, out = ((c0 x + c1 m0) + c2 D1) + c3 D2
 *   form 3: multistep third (:835-856): D1_0 = c4 (m0 - m1), D1_1 = c5 (m1 - m2), dd = D1_0 - D1_1, D1 = D1_0 + c6 dd, D2 = c7 dd,
 *           out = ((c0 x + c1 m0) + c2 D1) + c3 D2 */
int sdmi_dpm_update(int form, const float* x, const float* m0, const float* m1, const float* m2, const float* c9, float* out, int64_t n,
                    void* stream);

/* Dynamic-thresholding scale (:395-397): s_out[b] = max(quantile_0.995(|x0[b]|), max_val) by a radix select per row (no sort, no host
 * sync, integer atomics only: the same bits for every launch and run); torch.quantile's rank 0.995 (row - 1) in fp32 and its lerp.
 * A row with a NaN gives NaN.  stats_out (optional, [B, 2]): the two order statistics.  row <= 2^24. */
int sdmi_dpm_threshold_scale(const float* x0, int B, int64_t row, float max_val, float* s_out, float* stats_out, void* stream);

/* Adaptive error (:952-954): E[0] = max_b sqrt(mean(((x_higher - x_lower) / max(atol, rtol max(|x_lower|, |x_prev|)))^2)), left on the
 * device; two launches, a summation tree fixed by `row` alone.  ws: at least the _ws_floats floats of device memory. */
int64_t sdmi_dpm_adaptive_error_ws_floats(int B, int64_t row);
int sdmi_dpm_adaptive_error(const float* x_higher, const float* x_lower, const float* x_prev, float atol, float rtol, int B, int64_t row,
                            float* ws, int64_t ws_floats, float* E, void* stream);

/* ---- first stage (AutoencoderKL): SURVEY.md 8 f-1 ---------------------------------------------------------------
 * Replaces instantiate_from_config(first_stage_config) (ddpm.py:462-467) for inference:
 * `decode_first_stage` (ddpm.py:705-763) -> AutoencoderKL.decode (autoencoder.py:330-333) -> Decoder.forward
 * (ldm/modules/diffusionmodules/model.py:528-568), and `encode_first_stage` (ddpm.py:825-863) ->
 * AutoencoderKL.encode (autoencoder.py:324-328) -> Encoder.forward (model.py:427-460). */
typedef struct sdmi_vae sdmi_vae;
/* ddconfig of configs/stable-diffusion/v1-inference.yaml:51-65 (attn_resolutions = [], dropout 0, double_z) + embed_dim
 * (attn_resolutions != []: sdmi_vae_create_attn, below; z_channels <= 16 (or 32 / 64), embed_dim <= 16 (or 32 / 64), in_channels <= 16,
 * out_ch <= 8; n_levels <= 8) */
typedef struct sdmi_vae_cfg {
  int32_t ch;
  int32_t out_ch;
  int32_t n_levels;
  int32_t ch_mult[8];
  int32_t num_res_blocks;
  int32_t in_channels;
  int32_t z_channels;
  int32_t embed_dim;
} sdmi_vae_cfg;
/* parts: 1 = decoder (+post_quant_conv), 2 = encoder (+quant_conv), 3 = both */
int sdmi_vae_create(const sdmi_vae_cfg* cfg, int parts, sdmi_vae** out);
/* First stages beyond AutoencoderKL (additive; sdmi_vae_cfg is unchanged).  VQModelInterface of the latent-inpainting model
 * (autoencoder.py:14-283 with taming's VectorQuantizer2, legacy form): double_z = 0, mid_attn = 0 (attn_type 'none'), n_embed = 8192.
 *   double_z   1: the encoder emits 2 z_channels and quant_conv 2 embed_dim (AutoencoderKL); 0: z_channels / embed_dim (VQModel:
 *              sdmi_vae_encode then writes h = quant_conv(encoder(x)) [B, embed_dim, H/f, W/f], autoencoder.py:269-272)
 *   mid_attn   1: mid.attn_1 in encoder and decoder (attn_type 'vanilla'); 0: none (attn_type 'none')
 *   n_embed    > 0: the codebook `quantize.embedding.weight` [n_embed, embed_dim] is a weight of the decoder part; 0: none
 * sdmi_vae_create(cfg, parts, out) = sdmi_vae_create_ext(cfg, NULL, parts, out) (NULL = {1, 1, 0}). */
typedef struct sdmi_vae_ext {
  int32_t double_z;
  int32_t mid_attn;
  int32_t n_embed;
} sdmi_vae_ext;
int sdmi_vae_create_ext(const sdmi_vae_cfg* cfg, const sdmi_vae_ext* ext, int parts, sdmi_vae** out);
/* The first stage's precision, fixed for the handle's lifetime (additive; sdmi_vae_cfg and sdmi_vae_ext are unchanged):
 *   SDMI_PRECISION_MIXED  what sdmi_vae_create / sdmi_vae_create_ext create: fp16 MFMA operands, fp32 accumulation and stream
 *   SDMI_PRECISION_FULL   every MFMA operand of the ResBlocks, the Upsample / Downsample convs and the mid-block attention is a
 *                         split-fp16 pair (three MFMA passes); the attention is one split-fp16 flash launch at d = the mid width
 *                         (sdmi_k_attention_split16's head dims).  A mid width with mid_attn = 1 that no split-fp16 attention
 *                         kernel instantiates is refused here, by name.  Same weight keys and shapes, a larger workspace.
 * ext = NULL is {1, 1, 0}.  sdmi_vae_create_ext(cfg, ext, parts, out) = sdmi_vae_create_precision(cfg, ext, parts, SDMI_PRECISION_MIXED, out). */
int sdmi_vae_create_precision(const sdmi_vae_cfg* cfg, const sdmi_vae_ext* ext, int parts, int precision, sdmi_vae** out);
int sdmi_vae_precision(const sdmi_vae* h);        /* SDMI_PRECISION_*, or -1 for a null handle */
/* First stages with attention at resolution levels: `attn_resolutions` of the ddconfig (additive; sdmi_vae_cfg and sdmi_vae_ext are
 * unchanged).  KL-f16 of the retrieval-augmented model (models/first_stage_models/kl-f16: ch 128, ch_mult [1,1,2,2,4], z_channels 16,
 * embed_dim 16, attn_resolutions [16]) is attn_level_mask = 1 << 4.
 *   attn_level_mask   bit l set: an AttnBlock (one head of d = ch * ch_mult[l]) follows EVERY ResBlock of level l -- encoder.down.l.attn.i
 *                     for i < num_res_blocks, decoder.up.l.attn.i for i <= num_res_blocks (model.py:404-405, 442-444, 517-518, 553-555).
 *                     The caller resolves attn_resolutions to levels: level l runs at resolution >> l.  Bits at or past n_levels are refused.
 * A handle with a non-zero mask runs every attention block in mixed precision, the mid block's included, as GroupNorm -> q / k / v GEMMs ->
 * ONE flash launch (sdmi_k_attention's kernels, d = 512 on KL-f16) -> proj_out + residual: no N x N score buffer, any latent size.  In
 * SDMI_PRECISION_FULL the blocks are the split-fp16 ones of sdmi_vae_create_precision.  Every attention width of the handle that its mode has
 * no kernel for (mixed: sdmi_k_attention's head dims; full: sdmi_k_attention_split16's) is refused here, by level.
 * z_channels and embed_dim may be up to 16 (double_z: a 32-channel encoder.conv_out and a 32 -> 32 quant_conv), or 32 or 64 (KL-f32 of
 * models/first_stage_models/kl-f32: ch_mult [1,1,2,2,4,4], z_channels 64, embed_dim 64, attn_resolutions [16, 8] = mask 0b110000; its ends
 * run sdmi_k_conv_in64 / sdmi_k_conv_out128 / sdmi_k_pointwise_nchw128's launches).  A codebook first stage (ext->n_embed > 0, double_z 0:
 * VQ-f8 with attn_resolutions [32] = mask 1 << 3, VQ-f16 with [16] = 1 << 4) takes a mask like any other.
 * In SDMI_PRECISION_MIXED a stage of six or more levels runs its decoder's mid block and its levels >= 4 (1 / 16 of the image resolution and
 * below) with split-fp16 operands, as SDMI_PRECISION_FULL runs every layer; stages of up to five levels have fp16 operands throughout.
 * A handle with mask 0 keeps the GEMM / softmax / GEMM mid attention where H * W % 64 == 0 and takes the flash form elsewhere.
 * sdmi_vae_create_precision(cfg, ext, parts, precision, out) = sdmi_vae_create_attn(cfg, ext, parts, precision, 0, out): mask 0 launches
 * exactly what that entry always launched. */
int sdmi_vae_create_attn(const sdmi_vae_cfg* cfg, const sdmi_vae_ext* ext, int parts, int precision, uint32_t attn_level_mask,
                         sdmi_vae** out);
/* VQModelInterface.decode(h, force_not_quantize) (autoencoder.py:274-283): quantize = 1 replaces z_scale * z by its nearest
 * codebook entry first (sdmi_k_vq_quantize's arithmetic), then post_quant_conv -> decoder; quantize = 0 is sdmi_vae_decode.
 * The workspace is sdmi_vae_decode_workspace_bytes. */
int sdmi_vae_decode_vq(sdmi_vae* h, const float* z, float z_scale, int quantize, float* img, int B, int H, int W, void* workspace,
                       int64_t workspace_bytes, void* stream);
int sdmi_vae_destroy(sdmi_vae* h);
/* the state_dict keys the handle expects (= AutoencoderKL.state_dict() of the chosen parts, without `loss.*`) */
int sdmi_vae_num_weights(const sdmi_vae* h);
int sdmi_vae_weight_info(const sdmi_vae* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim);
int sdmi_vae_set_weight(sdmi_vae* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream);
int sdmi_vae_finalize(sdmi_vae* h);
/* z fp32 [B, embed_dim, H, W] -> img fp32 [B, out_ch, H*f, W*f], f = 2^(n_levels-1); z is multiplied by z_scale first
 * (decode_first_stage passes 1/scale_factor, ddpm.py:713; AutoencoderKL.decode passes 1) */
int64_t sdmi_vae_decode_workspace_bytes(sdmi_vae* h, int B, int H, int W);
int sdmi_vae_decode(sdmi_vae* h, const float* z, float z_scale, float* img, int B, int H, int W, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* img fp32 [B, in_channels, H, W] (H, W multiples of f) -> moments fp32 [B, 2*embed_dim, H/f, W/f]: the parameters of
 * DiagonalGaussianDistribution (mean | logvar), ldm/modules/distributions/distributions.py:24-33 */
int64_t sdmi_vae_encode_workspace_bytes(sdmi_vae* h, int B, int H, int W);
int sdmi_vae_encode(sdmi_vae* h, const float* img, float* moments, int B, int H, int W, void* workspace,
                    int64_t workspace_bytes, void* stream);


/* ---- text encoder (FrozenCLIPEmbedder): SURVEY.md 8 f-2 ----------------------------------------------------------
 * Replaces `self.transformer(input_ids=tokens).last_hidden_state` of FrozenCLIPEmbedder.forward
 * (ldm/modules/encoders/modules.py:155-160); `self.transformer` is transformers' CLIPTextModel (transformers==4.19.2,
 * environment.yaml:25; models/clip/modeling_clip.py).  The tokenizer stays on the host. */
typedef struct sdmi_clip sdmi_clip;
/* CLIPTextConfig fields (openai/clip-vit-large-patch14: 49408, 768, 3072, 12, 12, 77); hidden_act = quick_gelu */
typedef struct sdmi_clip_cfg {
  int32_t vocab_size;
  int32_t hidden_size;
  int32_t intermediate_size;
  int32_t num_layers;
  int32_t num_heads;
  int32_t max_positions;
} sdmi_clip_cfg;
int sdmi_clip_create(const sdmi_clip_cfg* cfg, sdmi_clip** out);
/* The handle's precision, fixed at creation (SDMI_PRECISION_* as for the UNet and the first stage; any other value is refused):
 *   SDMI_PRECISION_MIXED  what sdmi_clip_create creates: every GEMM and attention operand rounded to fp16 once
 *   SDMI_PRECISION_FULL   every MFMA operand a split-fp16 pair (three passes): Linear weights packed [hi | hi | lo], LayerNorm, the
 *                         per-head scatter and quick_gelu write hi / lo, the causal self-attention runs on
 *                         sdmi_k_attention_split16_causal.  Same state_dict keys and shapes; a larger workspace.  A head dim
 *                         (hidden_size / num_heads) outside {32, 64, 128} is refused at creation with a message that names it.
 * sdmi_clip_create(cfg, out) = sdmi_clip_create_precision(cfg, SDMI_PRECISION_MIXED, out). */
int sdmi_clip_create_precision(const sdmi_clip_cfg* cfg, int precision, sdmi_clip** out);
int sdmi_clip_precision(const sdmi_clip* h);      /* SDMI_PRECISION_*, or -1 for a null handle */
int sdmi_clip_destroy(sdmi_clip* h);
/* state_dict keys of CLIPTextModel as transformers 4.19.2 names them (`text_model.embeddings...`, `text_model.encoder
 * .layers.N...`, `text_model.final_layer_norm...`), i.e. the checkpoint's `cond_stage_model.transformer.` sub-tree */
int sdmi_clip_num_weights(const sdmi_clip* h);
int sdmi_clip_weight_info(const sdmi_clip* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim);
int sdmi_clip_set_weight(sdmi_clip* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream);
int sdmi_clip_finalize(sdmi_clip* h);
int64_t sdmi_clip_workspace_bytes(sdmi_clip* h, int B, int L);
/* ids: int64 [B, L] token ids (device); out: fp32 [B, L, hidden_size] = last_hidden_state */
int sdmi_clip_forward(sdmi_clip* h, const int64_t* ids, float* out, int B, int L, void* workspace, int64_t workspace_bytes,
                      void* stream);
/* OpenAI CLIP's encode_text (clip/model.py), what FrozenCLIPTextEmbedder runs (ldm/modules/encoders/modules.py:165-194).  A handle
 * created here declares one more weight behind the tower's, `text_projection.weight` [projection_dim, hidden_size] (the key and
 * orientation of transformers' CLIPTextModelWithProjection; no bias); sdmi_clip_create / sdmi_clip_create_precision handles keep their
 * weight lists and refuse sdmi_clip_text_embeds by name.  sdmi_clip_forward works on both. */
int sdmi_clip_create_projection(const sdmi_clip_cfg* cfg, int projection_dim, int precision, sdmi_clip** out);
int sdmi_clip_projection_dim(const sdmi_clip* h);  /* 0 for a handle without a projection, -1 for a null handle */
int64_t sdmi_clip_text_embeds_workspace_bytes(sdmi_clip* h, int B, int L);
/* ids: int64 [B, L] (device); out: fp32 [B, projection_dim] = last_hidden_state[b, argmax(ids[b, :])] @ text_projection.weight^T, the FIRST
 * maximum as clip/model.py takes it (no fixed eos id), divided by its L2 norm when normalize != 0.  Two launches behind the tower (gather + projection, normalisation); the
 * projection's operands are those of the handle's precision (fp16 once, or split-fp16 pairs with the three products of that mode). */
int sdmi_clip_text_embeds(sdmi_clip* h, const int64_t* ids, float* out, int B, int L, int normalize, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ---- text encoder of the LAION-400M model (BERTEmbedder) -------------------------------------------------------
 * Replaces `self.transformer(tokens, return_embeddings=True)` of BERTEmbedder.forward (ldm/modules/encoders/modules.py:
 * 80-103): x_transformer.TransformerWrapper(attn_layers=Encoder(dim, depth)) -- token + absolute position embedding,
 * `depth` pre-norm (attention, feed-forward) pairs (bias-free q/k/v of width heads*dim_head, non-causal, no mask; exact-erf
 * GELU), final LayerNorm.  The tokenizer stays on the host. */
typedef struct sdmi_bert sdmi_bert;
/* LAION-400M (txt2img-1p4B-eval.yaml): 30522, 1280, 32, 8, 64, 5120, 77.  dim and ff_inner multiples of 64, dim_head one
 * the attention kernel has (32, 40, 64, 80, 128, 160) */
typedef struct sdmi_bert_cfg {
  int32_t vocab_size;
  int32_t dim;
  int32_t depth;
  int32_t heads;
  int32_t dim_head;
  int32_t ff_inner;
  int32_t max_seq_len;
} sdmi_bert_cfg;
int sdmi_bert_create(const sdmi_bert_cfg* cfg, sdmi_bert** out);
/* As sdmi_clip_create_precision: SDMI_PRECISION_FULL runs every MFMA operand as a split-fp16 pair (the non-causal
 * sdmi_k_attention_split16, which has every dim_head of the list above; the exact-erf GELU writes hi / lo).  Same keys and shapes, a
 * larger workspace; any other precision value is refused.  sdmi_bert_create(cfg, out) = sdmi_bert_create_precision(cfg, SDMI_PRECISION_MIXED, out). */
int sdmi_bert_create_precision(const sdmi_bert_cfg* cfg, int precision, sdmi_bert** out);
int sdmi_bert_precision(const sdmi_bert* h);      /* SDMI_PRECISION_*, or -1 for a null handle */
int sdmi_bert_destroy(sdmi_bert* h);
/* state_dict keys of TransformerWrapper (`token_emb.weight`, `pos_emb.emb.weight`, `attn_layers.layers.N...`, `norm...`,
 * `to_logits...`), i.e. the checkpoint's `cond_stage_model.transformer.` sub-tree.  `to_logits.*` is shape-checked and
 * dropped (return_embeddings=True never applies it); finalize does not require it. */
int sdmi_bert_num_weights(const sdmi_bert* h);
int sdmi_bert_weight_info(const sdmi_bert* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim);
int sdmi_bert_set_weight(sdmi_bert* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream);
int sdmi_bert_finalize(sdmi_bert* h);
int64_t sdmi_bert_workspace_bytes(sdmi_bert* h, int B, int L);
/* ids: int64 [B, L] token ids (device), B <= 64, L <= max_seq_len; out: fp32 [B, L, dim] */
int sdmi_bert_forward(sdmi_bert* h, const int64_t* ids, float* out, int B, int L, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* ---- CLIP image encoder (vision tower) ------------------------------------------------------------------------------
 * transformers' CLIPVisionModelWithProjection: the tower of the safety checker that scripts/txt2img.py:check_safety and
 * scripts/img2img.py run on every decoded image, and of FrozenClipImageEmbedder (ldm/modules/encoders/modules.py:197-228).
 * Mixed precision only (fp16 MFMA operands, fp32 accumulation and residual stream).  Refused at creation, each with a message
 * that names it: hidden_size or intermediate_size off the 64 grid, a head dim the attention kernel does not have,
 * image_size % patch_size != 0, more than 1024 tokens; at run time B > 64. */
typedef struct sdmi_vit sdmi_vit;
/* CLIPVisionConfig fields + projection_dim (openai/clip-vit-large-patch14: 224, 14, 1024, 4096, 24, 16, 768); hidden_act = quick_gelu */
typedef struct sdmi_vit_cfg {
  int32_t image_size;
  int32_t patch_size;
  int32_t hidden_size;
  int32_t intermediate_size;
  int32_t num_layers;
  int32_t num_heads;
  int32_t projection_dim;
} sdmi_vit_cfg;
int sdmi_vit_create(const sdmi_vit_cfg* cfg, sdmi_vit** out);
int sdmi_vit_destroy(sdmi_vit* h);
/* state_dict keys of CLIPVisionModelWithProjection: `vision_model.embeddings.{class_embedding, patch_embedding.weight,
 * position_embedding.weight}`, `vision_model.pre_layrnorm.*` (the reference's spelling), `vision_model.encoder.layers.N.*`,
 * `vision_model.post_layernorm.*`, `visual_projection.weight` */
int sdmi_vit_num_weights(const sdmi_vit* h);
int sdmi_vit_weight_info(const sdmi_vit* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim);
int sdmi_vit_set_weight(sdmi_vit* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream);
int sdmi_vit_finalize(sdmi_vit* h);
int64_t sdmi_vit_workspace_bytes(sdmi_vit* h, int B);
/* pixel_values: fp32 [B, 3, image_size, image_size] (device), B <= 64.  last_hidden (optional): fp32 [B, T, hidden_size], the encoder
 * output, T = 1 + (image_size / patch_size)^2; pooled (optional): fp32 [B, hidden_size] = post_layernorm(last_hidden[:, 0]);
 * image_embeds: fp32 [B, projection_dim] = visual_projection(pooled) */
int sdmi_vit_forward(sdmi_vit* h, const float* pixel_values, float* last_hidden_or_null, float* pooled_or_null, float* image_embeds, int B,
                     void* workspace, int64_t workspace_bytes, void* stream);
/* The tower's streaming kernels.  patchify: fp32 [B, 3, S, S] -> fp16 rows [B (S / p)^2][Kp], column (c, ky, kx) of patch (py, px) in the
 * order of the conv weight's own [3][p][p] tail, Kp = 3 p^2 rounded up to a multiple of 64 (sdmi_k_vit_kpad), pad columns zero.
 * embed: out fp32 [B, T, C], row 0 = class_embedding + position_embedding[0], row 1 + i = patch row i + position_embedding[1 + i].
 * preprocess (FrozenClipImageEmbedder.preprocess): fp32 [B, 3, H, W] in [-1, 1] -> bicubic resize to S x S (align_corners=True,
 * A = -0.75, border taps clamped, no antialiasing), (x + 1) / 2, then (x - mean) / std with CLIP's constants. */
int sdmi_k_vit_kpad(int patch_size);
int sdmi_k_vit_patchify(const float* pixel_values, void* out_f16, int B, int S, int p, void* stream);
int sdmi_k_vit_embed(const float* patch, const float* class_embedding, const float* position_embedding, float* out, int B, int T, int C,
                     void* stream);
int sdmi_k_vit_preprocess(const float* x, float* out, int B, int H, int W, int S, void* stream);
/* StableDiffusionSafetyChecker.forward behind the tower, all fp32: every vector L2-normalised, all cosines; per image adjustment = 0; for each
 * special-care concept in index order s = round3(cos - threshold + adjustment) (three decimals, half to even), s > 0 sets adjustment = 0.01;
 * for each concept s = round3(cos - threshold + adjustment), bad if s > 0; has_nsfw[b] = any bad.  image_embeds [B, E], concept_embeds
 * [Nc, E], special_care_embeds [Ns, E], thresholds [Nc] / [Ns]; outputs int32 has_nsfw [B] and the rounded scores [B, Nc] / [B, Ns].
 * 1 <= Nc <= 64, 0 <= Ns <= 64 (the special-care pointers may be NULL when Ns = 0), E % 4 == 0, E <= 8192. */
int sdmi_k_safety_head(const float* image_embeds, const float* concept_embeds, const float* special_care_embeds,
                       const float* concept_thresholds, const float* special_care_thresholds, int32_t* has_nsfw, float* concept_scores,
                       float* special_care_scores, int B, int Nc, int Ns, int E, void* stream);

/* ---- the safety checker's feature extractor (scripts/txt2img.py:26-29, 88-90) --------------------------------------------
 * CLIPFeatureExtractor on the device: numpy_to_pil's uint8 conversion, PIL's 8-bit bicubic Image.resize of the shortest side to `size`
 * (the other side int(size * long / short)), the centre crop (top = (rh - crop) / 2, left = (rw - crop) / 2), / 255 and (x - mean) / std.
 * The resized uint8 image equals Pillow's bit for bit; the float stage is three correctly rounded fp32 operations.
 * Additive entry points: no existing struct or call changes, SDMI_ABI_VERSION stays as it is.
 *
 * Host side (no GPU): Pillow's coefficient tables of one axis in -> out, computed in double in Pillow's evaluation order.
 * sdmi_fe_ksize: taps per output index, (int)ceil(2 max(in / out, 1)) * 2 + 1, or -1 for sizes below 1.  sdmi_fe_coeffs fills
 * bounds [out][2] = {xmin, xmax} (the taps of output index xx read source indices xmin .. xmin + xmax - 1, all inside [0, in)) and
 * kk [out][ksize], the bicubic (a = -0.5) weights normalised to sum 1 and rounded to 22 fraction bits; entries x >= xmax are 0. */
int sdmi_fe_ksize(int in, int out);
int sdmi_fe_coeffs(int in, int out, int32_t* bounds, int32_t* kk);
int sdmi_fe_output_size(int H, int W, int size, int* rh, int* rw);
/* Source kinds of sdmi_k_clip_feature_extract.  Values outside a kind's range are clamped: a float becomes
 * clamp(rint(x * 255), 0, 255) (fp32 multiply, round half to even: numpy_to_pil's (x * 255).round().astype(uint8) wherever that is defined);
 * the raw kind applies clamp((x + 1) / 2, 0, 1) first, in the fp32 operation order of scripts/txt2img.py:314. */
#define SDMI_FE_SRC_U8_NHWC 0       /* uint8 [B, H, W, 3] */
#define SDMI_FE_SRC_F32_NHWC 1      /* fp32 [B, H, W, 3] in [0, 1] (the script's x_image) */
#define SDMI_FE_SRC_F32_NCHW 2      /* fp32 [B, 3, H, W] in [0, 1] */
#define SDMI_FE_SRC_F32_NCHW_RAW 3  /* fp32 [B, 3, H, W] in [-1, 1]: the decode_first_stage output itself */
/* bytes of the horizontal pass's uint8 rows (0 when the width does not change), or -1 with the error set */
int64_t sdmi_fe_workspace_bytes(int B, int H, int W, int size, int crop);
/* One batch of equal-sized device images -> pixel_values fp32 [B, 3, crop, crop] and, when out_u8_or_null is given, the resized and cropped
 * uint8 image [B, crop, crop, 3].  h_* : the device copies of sdmi_fe_coeffs(W, rw), v_* : of sdmi_fe_coeffs(H, rh), (rh, rw) =
 * sdmi_fe_output_size(H, W, size); the tables of an axis that keeps its size are not read and may be NULL.  mean3 / std3: host arrays.
 * At most two launches (horizontal; vertical + crop + normalise), no atomics, the source is only read.  Only the crop window is computed:
 * its columns, and the source rows its vertical pass reads.  Refused, launching nothing, each with a message that names it: crop > size
 * (the processor's padding), C != 3, sizes below 1, tables whose ksize is not sdmi_fe_ksize of the sizes given, a horizontal ksize above
 * 255, a workspace smaller than sdmi_fe_workspace_bytes. */
int sdmi_k_clip_feature_extract(const void* src, int src_kind, int B, int C, int H, int W, int size, int crop, const int32_t* h_bounds,
                                const int32_t* h_kk, int h_ksize, const int32_t* v_bounds, const int32_t* v_kk, int v_ksize,
                                const float* mean3, const float* std3, void* workspace, int64_t workspace_bytes, float* pixel_values,
                                void* out_u8_or_null, void* stream);

/* ---- exact k-nearest-neighbour search (retrieval conditioning) -------------------------------------------------------
 * Replaces `Searcher.search` of scripts/knn2img.py (scann's score_brute_force with dot_product between L2-normalised vectors): an exact
 * maximum-cosine search over a database of raw fp32 embeddings kept on the device, one copy of the rows plus one inverse norm per row.
 * Results are ordered by descending score, ties go to the LOWER row index (a stable argsort of -score).  Exact arithmetic in fp32 with
 * one fixed summation order: a (query, row) score has the same bits wherever the row sits.  Limits, each refused with a message that
 * names it: D % 4 == 0, D <= 1024, 1 <= B <= 64, 1 <= k <= 64, k <= rows, rows < 2^31 (row offsets are 64-bit).
 * Additive entry points: no existing struct or call changes, SDMI_ABI_VERSION stays as it is. */
typedef struct sdmi_knn sdmi_knn;
/* allocates capacity * (D + 1) floats; refused when that exceeds the free device memory (the message names both sizes) */
int sdmi_knn_create(int D, int64_t capacity_rows, sdmi_knn** out);
int sdmi_knn_destroy(sdmi_knn* h);
/* raw (unnormalised) rows [n][D], host or device memory, copied to rows first_row .. first_row + n; chunks arrive in order
 * (first_row <= rows set so far), so a multi-file database needs no second host copy */
int sdmi_knn_set_rows(sdmi_knn* h, int64_t first_row, int64_t n, const float* rows, void* stream);
/* inverse norms on the device; synchronises the stream.  A row with a zero or non-finite norm is an error that names the first such row */
int sdmi_knn_finalize(sdmi_knn* h, void* stream);
int64_t sdmi_knn_rows(const sdmi_knn* h);         /* rows set so far, or -1 for a null handle */
int sdmi_knn_dim(const sdmi_knn* h);
int64_t sdmi_knn_workspace_bytes(sdmi_knn* h, int B, int k);
/* queries: fp32 [B, D] (device), normalised on the device.  idx_out int32 [B, k], score_out fp32 [B, k] = (q / |q|) . x / |x|;
 * nn_out (optional) fp32 [B, k, D] = x[idx] / |x[idx]|.  Launches: scan, merge (two stages above 64 slabs), gather. */
int sdmi_knn_search(sdmi_knn* h, const float* queries, int B, int k, int32_t* idx_out, float* score_out, float* nn_out_or_null,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* the sampler's context: c fp32 [B, 1, D] (device) is the query AND slot 0 of c_out fp32 [B, 1 + k, D] (copied bit for bit); slots 1 .. k
 * are the normalised neighbours: `torch.cat([c, nn_embeddings], dim=1)` with no host round trip.  idx_out / score_out as above. */
int sdmi_knn_condition(sdmi_knn* h, const float* c, int B, int k, float* c_out, int32_t* idx_out, float* score_out, void* workspace,
                       int64_t workspace_bytes, void* stream);
/* The kernels, with the slab size explicit.  inv_norm: fp32 [N].  scan: candidates [B][ceil(N / slab_rows)][k] (score, row index), unsorted,
 * lists of slabs with fewer than k rows padded with (-inf, INT32_MAX).  merge: candidates [B][n_lists][k] -> idx / score [B][k] in the
 * order above.  gather: out row b * (k + (c0 != NULL)) + slot at pitch ldo floats (ldo >= D, ldo % 4 == 0); c0 [B][D] or NULL. */
int sdmi_k_knn_inv_norm(const float* db, int64_t N, int D, float* inv_norm, void* stream);
int sdmi_k_knn_scan(const float* db, const float* inv_norm, int64_t N, int D, const float* queries, int B, int k, int64_t slab_rows,
                    float* cand_score, int32_t* cand_idx, void* stream);
int sdmi_k_knn_merge(const float* cand_score, const int32_t* cand_idx, int B, int n_lists, int k, int32_t* idx_out, float* score_out,
                     void* stream);
/* a plain read-only sweep of n_floats (a multiple of 4) with 16-byte loads: the bandwidth ceiling tools/bench_knn.py measures the scan
 * against.  sink: one float on the device, practically never written. */
int sdmi_k_knn_stream_read(const float* p, int64_t n_floats, float* sink, void* stream);
int sdmi_k_knn_gather(const float* db, const float* inv_norm, int64_t N, int D, const int32_t* idx, int B, int k, const float* c0_or_null,
                      float* out, int64_t ldo, void* stream);

/* ---- kernel-level entry points (parity tests and micro-benchmarks; same kernels the UNet uses) ---------- */
typedef struct sdmi_igemm_desc {
  const void* a0; const void* a1; const void* a2;   /* fp16 NHWC sources, channel concat [a0|a1|a2] (a1, a2 optional) */
  int32_t c0, c1, c2, lda0, lda1, lda2;
  int32_t B, Hin, Win, Hout, Wout, ksize, stride, up;
  const void* w;                        /* fp16 [N][K] from sdmi_k_pack_conv_weight(_src): K = ksize*ksize*(c0+c1+c2), ordered (64-ch chunk, ky, kx, ch); c0, c1, c2 % 32 == 0 */
  int32_t N;
  int32_t mode;                         /* 0 plain, 1 GEGLU (w/bias packed by sdmi_k_pack_geglu), 2 per-head scatter */
  const float* bias; const float* rowvec; int32_t ld_rowvec;
  const float* residual; int32_t ldr;
  float* out_f32; void* out_f16; int32_t ldo;
  void* seg_dst[3]; int32_t seg_kind[3];
  int32_t heads, dh, ntok, ntok_pad, segC;
  int32_t splitk;                       /* 1 none, 0 auto, >1 forced (plain mode; needs splitk_ws) */
  float* splitk_ws; int64_t splitk_ws_floats;   /* fp32 slabs: scratch, splitk * round_up(M, BM) * round_up(N, BN) floats cover every
                                                   layout (whole tiles in the MFMA register order -- the default since round 4,
                                                   SDMI_SLAB_TILED -- or [splitk][M][N]; see also splitk_cnt) */
  int32_t tile;                         /* -1 auto (tuning table); BMxBN/waves/LDS-DMA stages: 0 128x128/4/2, 1 128x64/4/2,
                                           2 64x64/4/2, 3 256x128/8/2, 4 128x64/4/3, 5 64x64/4/3, 6 256x128/8/3, 7 128x128/4/3,
                                           8 64x128/4/3, 9 128x128/8/3, 10 64x64/4/4, 11 128x256/8/2, 12 64x256/4/3, 13 256x64/4/3;
                                           halo-staged 3x3 conv (stride 1, pad 1, width 16/32/64, whole-row tiles):
                                           14 256x64/8/5, 15 256x128/8/3, 16 128x64/4/8, 17 128x128/4/5;
                                           deep rings (generic): 18 64x64/4/8, 19 64x128/4/6, 20 128x64/4/6, 21 128x128/8/4 */
  int32_t dma;                          /* -1 default, 0 register staging, 1 LDS-DMA */
  int32_t asym_pad;                     /* 3x3 only: 0 = zero pad 1 on every side; 1 = pad right/bottom only, i.e.
                                           F.pad(x,(0,1,0,1)) + conv(padding=0) of the VAE Downsample (model.py:72-76) */
  /* optional (mode 0, Hout*Wout % 32 == 0): GroupNorm(32) statistics of the output for up to two consuming GroupNorms
   * (util.py:199-216), accumulated by the epilogue / the split-K reduce into int64 fixed-point words
   * gn_acc[t][B][32 groups][8 slots][16] (one 128-byte line per slot; words 0..3 = {sum int, sum frac * 2^40, sumsq int,
   * sumsq frac * 2^40}; zero them first);
   * the output is channels [gn_cbase, gn_cbase + N) of that GroupNorm's input, gn_cpg channels per group */
  int32_t gn_n; void* gn_acc[2]; int32_t gn_cpg[2]; int32_t gn_cbase[2];
  /* optional: ints zeroed before the first launch (the kernels leave them zero); the GroupNorm-applying split-K reduction
   * below keeps its grid-barrier words in the last 576 of them */
  int32_t* splitk_cnt; int32_t splitk_cnt_ints;
  /* split-fp16 dense GEMM (csrc/gemm_split16.hip; ksize 1, mode 0): a0 = high halves and a1 = low halves of the fp32
   * activation ([M][c0] each, sdmi_k_cast_f16), w = sdmi_k_pack_split3 ([N][3 c0] = [hi | hi | lo]);
   * out = a_hi w_hi^T + a_lo w_hi^T + a_hi w_lo^T from four operand tiles per 64-channel chunk.  tile: -1, 0, 1, 2, 4, 5, 8, 10 */
  int32_t split16;
  /* LayerNorm folded into the consuming GEMM (attention.py:211-215; csrc/common.h IGemmParams::lnp_out / lnf_*).
   * Producer (mode 0, out_f32 and out_f16, no split-K): out_f16 = fp16(f16_scale[n] * v) and lnp_out[(n / 32) * M + m] =
   * float2{sum, sum of squares} of row m over each 32-column block.  Consumer (dense, one source, no bias, no split-K): a0 =
   * that operand, lnf_part = its partials (lnf_npart = K / 32); every accumulator becomes
   * rstd_m * (acc - mean_m * lnf_cs[n]) + lnf_d[n] (vectors from sdmi_k_ln_fold_prep) before the mode's epilogue. */
  const float* f16_scale; float* lnp_out;
  const float* lnf_part; int32_t lnf_npart; float lnf_eps; const float* lnf_cs; const float* lnf_d;
  /* GroupNorm(32, pgn_eps) (+ SiLU) of the finished OUTPUT inside the split-K reduction (ABI 11; mode 0, N % 128 == 0: ResBlock
   * conv1 -> out_layers.0-1, openaimodel.py:225-227): with SDMI_REDUCE_GN_XCD=1, when the GEMM is split, the output is its one
   * GroupNorm statistics target and splitk_cnt is given, the reduction takes the statistics behind a grid barrier and stores
   * pgn_out [M][N] fp16 = SiLU(GN(v)); out_f32 is then written only with pgn_keep_f32.  *pgn_applied (host int, optional) is set
   * to 1 when that happened; when it is left 0 the launch was an ordinary one and pgn_out is untouched. */
  const float* pgn_gamma; const float* pgn_beta; float pgn_eps; int32_t pgn_silu;
  void* pgn_out; int32_t pgn_keep_f32; int32_t* pgn_applied;
  /* optional (ABI 12; mode 0, ldo % 4 == 0): fp16(v - float(fp16(v))) beside out_f16 -- the low half of the split-fp16 operand a
   * following split16 GEMM reads (the last FF-out of a SpatialTransformer feeds proj_out this way) */
  void* out_lo;
} sdmi_igemm_desc;
int sdmi_k_igemm(const sdmi_igemm_desc* d, void* stream);
/* ... with a 1x1 tail phase (a ResBlock's skip_connection inside conv2's launch, openaimodel.py:263-276): `d` is a stride-1 3x3 conv on a
 * halo-staged tile (tile 14..17, or -1 = tuning table; any other tile is an error, never a silent drop of the term), and
 *   out = conv3x3(a) + cat(t0, t1, t2)[M][tail_kt] tail_w[N][tail_kt]^T + epilogue,
 * accumulated in the conv's fp32 accumulators behind its chunk loop.  t0 .. t2: fp16 [M][tail_ld] buffers, tail_c (% 64 == 0) channels of each;
 * tail_kt = tail_c (t0 only, tail_w = fp16 [N][tail_c]) or 3 tail_c (t0 = hi, t1 = lo, t2 = hi against sdmi_k_pack_split3 weights).  Under
 * split-K the tail's k-tiles are dealt over the conv's splits in contiguous ranges (sdmi_k_tail_split_range: host arithmetic only).
 * Entry points beside sdmi_k_igemm rather than new sdmi_igemm_desc fields: the struct layout and SDMI_ABI_VERSION stay as they are. */
int sdmi_k_igemm_tail(const sdmi_igemm_desc* d, const void* t0, const void* t1, const void* t2, int tail_c, int tail_ld, const void* tail_w,
                      int tail_kt, void* stream);
int sdmi_k_tail_split_range(int nkt, int nsplit, int split, int* begin, int* end);
/* conv3x3(nearest x2 (a)) as the four 2x2 "phase" convs of ONE launch (csrc/igemm_kernel.h KIND_2X2): output pixel
 * (2i + a, 2j + c) of the upsampled map sees only source rows {i - 1 + a, i + a} and columns {j - 1 + c, j + c}, so each parity class is a 2x2
 * conv on the source map with summed taps -- 4 / 9 of the MACs.  `d` describes the reference op exactly as for sdmi_k_igemm (ksize 3, stride 1,
 * up 1, Hout = 2 Hin, Wout = 2 Win, one source of c0 % 64 == 0 channels, mode 0, no residual, splitk 0 or 1, tile -1 or a generic tile) except that
 * d->w = the weights sdmi_k_up_phase_weights derived: fp16 [4 phases = 2 a + c][N][4 c0], k' = ((ch / 64) * 4 + 2 dy + dx) * 64 + ch % 64.
 * sdmi_k_up_phase_weights(w_packed = sdmi_k_pack_conv_weight's fp16 [N][9 Cin], dst, N, Cin): the 1, 2 or 4 taps of the 3x3 window that fall on
 * one source pixel are added in fp32 in (ky, kx) order and rounded once to fp16.
 * Entry points beside sdmi_k_igemm rather than new sdmi_igemm_desc fields: the struct layout and SDMI_ABI_VERSION stay as they are. */
int sdmi_k_igemm_up_phase(const sdmi_igemm_desc* d, void* stream);
int sdmi_k_up_phase_weights(const void* w_packed_f16, void* dst_f16, int N, int Cin, void* stream);
/* GEGLU -> FF-out -> proj_out of a SpatialTransformer as ONE launch (ABI 12; csrc/rowchain.hip; ldm/modules/attention.py:58-64,214,
 * 258-261): out = residual + proj_out(t + FF(norm3(t))) for C = 320 channels, a workgroup per 32 token rows.
 * proj_out: the split-fp16 1x1 descriptor of the last GEMM (split16 = 1, c0 = N = C, w = sdmi_k_pack_split3, bias, residual, out_f32,
 * optional out_f16 copy / gn_* statistics targets; B * Hout * Wout = M rows, Hout * Wout % 32 == 0) -- a0 / a1 are not read.
 * ln_f16 [M][C] = fp16(gamma3 * t) and lnp [C / 32][M][2]: what the producer of t stored (f16_scale / lnp_out above);
 * csd: the GEGLU projection's LayerNorm-fold column terms (sdmi_k_ln_fold_prep over the packed weights, bias inside d) regrouped per
 * hidden chunk of C: [4][cs of 2C packed columns | d of the same 2C]; wgg [8C][C], wff2 [C][4C] fp16, bff2 [C], t [M][C] fp32. */
int sdmi_k_ff_tail(const sdmi_igemm_desc* proj_out, const void* ln_f16, const float* lnp, float ln_eps, const float* csd,
                   const void* wgg_f16, const void* wff2_f16, const float* bff2, const float* t, void* stream);
/* ... with the out-projection of the cross-attention in front (ABI 14; the same kernel; attention.py:213, 191-192): t += a Wo^T + bo in place
 * (a [M][C] fp16 = the attn2 output rows, wo [C][C] fp16, t [M][C] fp32 in / out), then the chain above over norm3(t) with ln_gamma = the norm3
 * weight (its bias lives in csd).  The same bits as sdmi_k_igemm (bias, residual = t, out_f32 = t, f16_scale, lnp_out) -> sdmi_k_ff_tail. */
int sdmi_k_st_tail(const sdmi_igemm_desc* proj_out, const void* a_f16, const void* wo_f16, const float* bo, float* t, const float* ln_gamma,
                   float ln_eps, const float* csd, const void* wgg_f16, const void* wff2_f16, const float* bff2, void* stream);
/* ResBlock in_layers / out_layers as ONE launch (ABI 15; csrc/gnconv.hip; ldm/modules/diffusionmodules/openaimodel.py:201-204, 225-231,
 * util.py:199-216): out = conv3x3(SiLU(GroupNorm32(cat(x0, x1)))) + bias (+ rowvec, + residual) for N = 320 output channels, a workgroup per
 * 32 pixels of an image row x all output channels (the input halo is normalised once per workgroup).
 * conv: the descriptor of the stride-1 3x3 convolution (ksize 3, c0 + c1 + c2 = Cin input channels, B, Hin = Hout, Win = Wout % 32 == 0,
 * w = sdmi_k_pack_conv, N = 320, mode 0, bias / rowvec / residual / out_f32 / out_f16 / gn_* as for sdmi_k_igemm) -- a0 .. a2 are not read;
 * x0 [B * H * W][c0], x1 [..][c1] (or NULL, c1 = 0) fp32 NHWC, 256 <= c0 + c1 <= 960, c0 % 64 == 0; gn_ws: sdmi_k_groupnorm_ws_floats(B, H * W)
 * floats of scratch (the statistics are computed by a statistics launch in front).  The same bits as sdmi_k_groupnorm (silu, fp16 out) ->
 * sdmi_k_igemm with splitk = 1. */
int sdmi_k_gn_conv3(const sdmi_igemm_desc* conv, const float* x0, const float* x1, int c0, int c1, float* gn_ws, int64_t gn_ws_floats,
                    const float* gn_gamma, const float* gn_beta, float gn_eps, void* stream);
/* GroupNorm-apply -> proj_in -> q | k | v of a SpatialTransformer as ONE launch (ABI 13; csrc/rowchain.hip; ldm/modules/attention.py:254-256,
 * 212, 170-176): t = proj_in(GroupNorm(x)) + b_in (fp32 [M][C], M = B * ntok), q | k | v = norm1(t) Wqkv^T scattered per head
 * (q, k: [B * heads][ntok][dh] fp16, vt: [B * heads][dh][ntok_pad] fp16) for C = 320 channels, a workgroup per 32 token rows.
 * x [M][C] fp32; gn_ws: sdmi_k_groupnorm_ws_floats(B, ntok) floats of scratch (the statistics are computed here, as sdmi_k_groupnorm does);
 * w_in3 = sdmi_k_pack_split3(proj_in weight) [C][3C]; ln_gamma = norm1 weight; wqkv [3C][C] fp16 (to_q | to_k | to_v rows);
 * lnf_cs / lnf_d [3C] = sdmi_k_ln_fold_prep(wqkv, norm1 weight, norm1 bias).  Same arithmetic, in the same order, as sdmi_k_groupnorm
 * (f16 + lo outputs) -> sdmi_k_igemm (split16, f16_scale, lnp_out) -> sdmi_k_igemm (mode 2, lnf_*): the outputs are the same bits. */
int sdmi_k_st_head(const float* x, float* gn_ws, int64_t gn_ws_floats, const float* gn_gamma, const float* gn_beta, float gn_eps,
                   const void* w_in3, const float* b_in, float* t, const float* ln_gamma, float ln_eps, const void* wqkv_f16,
                   const float* lnf_cs, const float* lnf_d, void* q, void* k, void* vt, int B, int ntok, int ntok_pad, int heads, int dh,
                   int C, void* stream);
/* The middle of a BasicTransformerBlock as ONE launch (ABI 13; same kernel; attention.py:212-213, 170, 191-192): t += a Wo^T + bo in place
 * (a [M][C] fp16 = the self-attention output, wo [C][C] fp16, t [M][C] fp32), q = norm2(t) Wq^T scattered per head ([B * heads][ntok][dh] fp16);
 * ln_gamma = norm2 weight, lnf_cs / lnf_d [C] = sdmi_k_ln_fold_prep(wq, norm2 weight, norm2 bias).  The same bits as sdmi_k_igemm (bias,
 * residual = t, out_f32 = t, f16_scale, lnp_out) -> sdmi_k_igemm (mode 2, lnf_*). */
int sdmi_k_st_mid(const void* a_f16, const void* wo_f16, const float* bo, float* t, const float* ln_gamma, float ln_eps, const void* wq_f16,
                  const float* lnf_cs, const float* lnf_d, void* q, int B, int ntok, int heads, int dh, int C, void* stream);
/* ... with the cross-attention behind to_q inside the same launch (ABI 16; attention.py:213, 170-193): ctx_k [B * heads][nkv][dh], ctx_vt
 * [B * heads][dh][nkv_pad] fp16 (the cached context projections, sdmi_k_igemm mode 2), scale = dh^-1/2, ao_out [B * ntok][C] fp16 = the attention
 * output rows (q is not written).  dh = 40, nkv <= 128.  The same bits as sdmi_k_st_mid -> sdmi_k_attention. */
int sdmi_k_st_mid_ctx(const void* a_f16, const void* wo_f16, const float* bo, float* t, const float* ln_gamma, float ln_eps, const void* wq_f16,
                      const float* lnf_cs, const float* lnf_d, const void* ctx_k, const void* ctx_vt, int nkv, int nkv_pad, float scale, void* ao_out,
                      int B, int ntok, int heads, int dh, int C, void* stream);
/* cs[n] = sum_k gamma[k] * w[n][k], d[n] = sum_k beta[k] * w[n][k] (+ bias[n]) over the PACKED fp16 weights w [N][ldw]
 * (first K columns of a row): the column terms of a GEMM that folds LayerNorm(gamma, beta) of its input rows */
int sdmi_k_ln_fold_prep(const void* w_f16, int N, int K, int ldw, const float* gamma, const float* beta, const float* bias,
                        float* cs, float* d, void* stream);
/* q [BH,nq,d], k [BH,nkv,d], vt [BH,d,nkv_pad] fp16 -> out fp16 [BH/heads, nq, heads*d]; attention.py:178-192.
 * nkv_pad is a multiple of 8 and >= nkv.  The pad columns nkv .. nkv_pad of every V^T row must be ZERO for head dims up to 160 (csrc/attn.hip,
 * and likewise for both halves in sdmi_k_attention_split16): the key tiles are staged past nkv, the score mask zeroes the probabilities of
 * those keys, and 0 x (a non-finite pad value) would still be NaN in the P V product.  The wide-head kernel (d = 192 .. 1024 in steps of 64,
 * csrc/attn_wide.hip) replaces the pad columns by zeros itself: they may hold anything there.  Producers inside the library keep the
 * contract (sdmi_k_igemm mode 2 into a cleared buffer, sdmi_k_split_heads kind 1 writes the pad tokens as zeros). */
int sdmi_k_attention(const void* q, const void* k, const void* vt, void* out, int BH, int heads, int nq, int nkv,
                     int nkv_pad, int d, float scale, void* stream);
/* The routing of sdmi_k_attention between its ring kernel and the one-pass kernel for at most 256 keys (csrc/attn_small.hip; d = 80 / 160,
 * non-causal): the one-pass kernel's waves per workgroup (1, 2 or 4) for this shape, or 0 where the ring kernel runs.  knob = the value of
 * SDMI_ATTN_SMALL: 0 the ring kernel everywhere, 1 the measured routing table (the default), 2 the one-pass kernel wherever it exists.  Host only. */
int sdmi_attn_small_takes(int d, int nq, int nkv, int causal, int knob);
/* split-fp16 attention (the full-precision mode): q / k / vt and their low halves q_lo / k_lo / vt_lo in the layouts above,
 * out / out_lo fp16 [BH/heads, nq, heads*d] = hi / lo of the fp32 result; d in {24, 32, 40, 48, 64, 80, 96, 128, 160} (csrc/attn_split16.hip)
 * or 192 .. 1024 in steps of 64 (csrc/attn_wide_split16.hip: four waves split d and sum their partial scores in a fixed order; like the
 * wide-head kernel of sdmi_k_attention it replaces the V^T pad columns nkv .. nkv_pad, hi and lo, by zeros itself).  Any other d fails
 * with a message that names it. */
int sdmi_k_attention_split16(const void* q, const void* q_lo, const void* k, const void* k_lo, const void* vt, const void* vt_lo, void* out,
                             void* out_lo, int BH, int heads, int nq, int nkv, int nkv_pad, int d, float scale, void* stream);
/* sdmi_k_attention_split16 with a causal mask (query i attends to keys <= i; nq == nkv = n): the self-attention of the full-precision
 * CLIP text encoder.  d in {32, 64, 128}; any other d fails with a message that names it.  The V^T pad columns n .. n_pad, hi and lo,
 * must be zero, as above. */
int sdmi_k_attention_split16_causal(const void* q, const void* q_lo, const void* k, const void* k_lo, const void* vt, const void* vt_lo,
                                    void* out, void* out_lo, int BH, int heads, int n, int n_pad, int d, float scale, void* stream);
/* sdmi_k_attention with a causal mask (query i attends to keys <= i; nq == nkv): CLIPTextModel's self-attention */
int sdmi_k_attention_causal(const void* q, const void* k, const void* vt, void* out, int BH, int heads, int n, int n_pad,
                            int d, float scale, void* stream);
/* GroupNorm(32) over cat(x0,x1) fp32 NHWC; any of the outputs may be NULL.  out_lo / raw_lo = fp16(v - fp16(v)):
 * the low halves of split-fp16 operands (3-pass 1x1 convs) */
int sdmi_k_groupnorm(const float* x0, const float* x1, int c0, int c1, int B, int HW, const float* gamma,
                     const float* beta, float eps, int silu, void* out_f16, float* out_f32, void* raw_f16, void* out_lo,
                     void* raw_lo, float* partial_ws, int64_t partial_floats, void* stream);
int64_t sdmi_k_groupnorm_ws_floats(int B, int HW);
/* sdmi_k_groupnorm with the scale-shift rows of a use_scale_shift_norm ResBlock (openaimodel.py:267-271) applied in the same launch:
 * y = SiLU((GN(x) gamma + beta) (1 + scale[b][c]) + shift[b][c]) feeds out_f16 / out_lo / out_f32; the raw copies are unchanged.
 * film: row b at film + b * film_ld holds scale in its first c0 + c1 floats and shift in the next c0 + c1 (th.chunk(emb_out, 2, dim=1));
 * film_ld = 0: one row shared by every sample; 16-byte aligned, film_ld % 4 == 0.  film = NULL: the same bits as sdmi_k_groupnorm. */
int sdmi_k_groupnorm_film(const float* x0, const float* x1, int c0, int c1, int B, int HW, const float* gamma, const float* beta, float eps,
                          int silu, const float* film, int film_ld, void* out_f16, float* out_f32, void* raw_f16, void* out_lo, void* raw_lo,
                          float* partial_ws, int64_t partial_floats, void* stream);
int sdmi_k_layernorm(const float* x, const float* gamma, const float* beta, void* out_f16, int M, int C, float eps,
                     void* stream);
int sdmi_k_cast_f16(const float* x, void* out_f16, void* out_lo, int64_t n, void* stream);
/* Producers of split-fp16 operands in the full-precision mode: fp32 in, hi / lo fp16 out.
 * split_heads: columns [col0, col0 + heads*dh) of src [B*ntok][ld] per head -- kind 0: [B*heads][ntok][dh] (q, k), kind 1: [B*heads][dh][ntok_pad]
 * (v^T, pad tokens zero).  geglu_split: src [M][2F] = proj(x) + bias -> value * gelu(gate) [M][F].  layernorm_split: as sdmi_k_layernorm. */
int sdmi_k_split_heads(const float* src, int ld, int col0, void* dst, void* dst_lo, int kind, int B, int ntok, int ntok_pad, int heads, int dh,
                       void* stream);
int sdmi_k_geglu_split(const float* src, int M, int F, void* out, void* out_lo, void* stream);
int sdmi_k_layernorm_split(const float* x, const float* gamma, const float* beta, void* out, void* out_lo, int M, int C, float eps, void* stream);
int sdmi_k_timestep_embedding(const int64_t* t_i64, const float* t_f32, float* out, int B, int dim, void* stream);
int sdmi_k_small_linear(const float* in, int ld_in, const float* w, const float* bias, float* out, int ld_out, int B,
                        int N, int K, int silu_in, void* stream);
int sdmi_k_conv_in(const float* x_nchw, const float* w_oihw, const float* bias, float* out_nhwc, int B, int Cin, int H,
                   int W, int Cout, void* stream);
int sdmi_k_conv_out(const float* h_nhwc, const float* w_ohwi, const float* bias, float* out_nchw, int B, int H, int W,
                    int Cin, int Cout, void* stream);
/* the same 3x3 output convolution for up to 32 outputs (the KL-f16 encoder's conv_out: 2 x 16 moment channels): one launch of
 * ceil(Cout / 8) slices of eight outputs for Cout > 8; up to 16 outputs it launches what sdmi_k_conv_out launches, which keeps refusing
 * more than 16 */
int sdmi_k_conv_out32(const float* h_nhwc, const float* w_ohwi, const float* bias, float* out_nchw, int B, int H, int W,
                      int Cin, int Cout, void* stream);
/* The wide latent ends of the first stages with 32 / 64 latent channels (KL-f32: decoder.conv_in 64 -> 512, encoder.conv_out 512 -> 128;
 * additive, fp32 like the entries above).
 *   sdmi_k_conv_in64     the 3x3 input convolution for up to 64 input channels: per output the bias, then k = ci*9 + ky*3 + kx ascending, an
 *                        order that depends on Cin alone.  Cin <= 16 launches what sdmi_k_conv_in launches (the same bits); sdmi_k_conv_in
 *                        keeps refusing more than 16.
 *   sdmi_k_conv_out128   the 3x3 output convolution for up to 128 outputs at Cin <= 512, Cin % 4 == 0: ceil(Cout / 8) slices of eight outputs
 *                        in one launch, the 4-pixel form where W % 4 == 0 and the pointers are 16-byte aligned, else one pixel per wave.  Up to
 *                        32 outputs it launches what sdmi_k_conv_out32 launches, which keeps refusing more than 32. */
int sdmi_k_conv_in64(const float* x_nchw, const float* w_oihw, const float* bias, float* out_nhwc, int B, int Cin, int H, int W,
                     int Cout, void* stream);
int sdmi_k_conv_out128(const float* h_nhwc, const float* w_ohwi, const float* bias, float* out_nchw, int B, int H, int W, int Cin,
                       int Cout, void* stream);
int sdmi_k_pack_conv_weight(const float* w_oihw, void* dst_f16, int O, int I, int KH, int KW, void* stream);
/* ... for A sources that are multiples of 32 channels (c0 + c1 + c2 == I, each % 32 == 0): the 64-channel chunks are numbered per source,
 * and the last chunk of a source of 32 (mod 64) channels is 32 wide (the kernels' half k-tile).  K = KH*KW*I stays dense.  With every source
 * a multiple of 64 the output equals sdmi_k_pack_conv_weight's, byte for byte.  sdmi_k_pack_conv_weight itself takes one source of I % 32 == 0. */
int sdmi_k_pack_conv_weight_src(const float* w_oihw, void* dst_f16, int O, int I, int KH, int KW, int c0, int c1, int c2, void* stream);
int sdmi_k_pack_conv_out(const float* w_oihw, float* dst_ohwi, int O, int I, void* stream);
/* [N][K] fp32 -> fp16 [N][3K] = [hi | hi | lo] for the 3-pass split-fp16 1x1 convs */
int sdmi_k_pack_split3(const float* w, void* dst_f16, int N, int K, void* stream);
/* [O][I][KH][KW] fp32 -> fp16 [O][3 KH KW I]: the 3-pass split-fp16 3x3 conv weights [w_hi | w_hi | w_lo], i.e. sdmi_k_pack_conv_weight
 * of the virtual [O][3 I][KH][KW] tensor, met by the K-concatenated operand a0 = hi, a1 = lo, a2 = hi (c0 = c1 = c2 = I); I % 32 == 0 */
int sdmi_k_pack_conv_split3(const float* w_oihw, void* dst_f16, int O, int I, int KH, int KW, void* stream);
/* first-stage helpers: 1x1 conv NCHW->NCHW on <= 32 input channels (input pre-scaled; Cin <= 16 and 17 .. 32 are two instantiations of
 * one kernel, per output: bias, then the input channels ascending); row softmax fp32 -> fp16 */
int sdmi_k_pointwise_nchw(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int HW,
                          float in_scale, void* stream);
/* ... on up to 128 input channels (KL-f32: quant_conv 128 -> 128, post_quant_conv 64 -> 64): a thread owns a pixel and a block of 16
 * output accumulators and walks the input channels once -- per output the bias, then the input channels ascending, as above.  Cin <= 32
 * launches what sdmi_k_pointwise_nchw launches, which keeps refusing more than 32. */
int sdmi_k_pointwise_nchw128(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int HW,
                             float in_scale, void* stream);
int sdmi_k_softmax_rows(const float* S, void* P_f16, int rows, int cols, float scale, void* stream);
/* exact-erf GELU (the BERT encoder's feed-forward activation): fp32 [n] -> fp16 [n], n % 4 == 0 */
/* The codebook quantizer of VectorQuantizer2 (legacy): per pixel of z' = z_scale * z (z fp32 NCHW [B, D, HW]) the first index of
 * min_n d = (sum z'^2 + sum e_n^2) - 2 z'.e_n over the codebook e [n_embed, D] fp32; zq (optional, NCHW) = z' + (e[idx] - z') in fp32;
 * idx (optional) int32 [B * HW].  norms_ws: n_embed floats of device scratch (receives sum e_n^2).  D in {1, 2, 3, 4, 8}. */
int sdmi_k_vq_quantize(const float* z, float z_scale, const float* codebook, float* norms_ws, int n_embed, int D, float* zq, int32_t* idx,
                       int B, int HW, void* stream);
/* 2x2 average pool (dir 1) / nearest x2 (dir -1) of fp32 NHWC [B, H, W, C] (C % 4 == 0): out_f32 and / or out_f16 (+ out_lo =
 * fp16(v - out_f16)), the resampling of the inpainting UNet's ResBlocks (openaimodel.py:253-259) */
int sdmi_k_resample2(const float* x, float* out_f32, void* out_f16, void* out_lo, int B, int H, int W, int C, int dir, void* stream);
/* The sliding windows of LatentDiffusion.split_input_params (ddpm.py:601-651, 902-984; additive, ABI 17).
 * sdmi_k_patch_unfold: windows l in [l0, l0 + nl) of x fp32 NCHW [B, Cx, H, W] -- and of c [B, Cc, H, W] behind them on the channel axis (the
 * torch.cat([x] + c_concat, 1) of DiffusionWrapper.forward; c NULL with Cc = 0) -- as rows (l - l0) * B + b of out [nl * B, Cx + Cc, kh, kw].
 * Window l starts at ((l / Lx) sy, (l % Lx) sx), Ly = (H - kh) / sy + 1, Lx = (W - kw) / sx + 1.  A copy: bit-exact.
 * sdmi_k_patch_fold: out [B, C, H uf / df, W uf / df] = sum_l w[l] o[l * B + b] / sum_l w[l] over the windows that cover an element, in
 * ascending l, fp32, no atomics (two runs give the same bits).  o [Ly Lx B, C, kh', kw'], w [Ly Lx, kh', kw'] with kh' = kh uf / df (window,
 * stride and output scaled alike: uf = vqf for decode_first_stage, df = vqf for encode_first_stage, both 1 for apply_model).  norm_only: o is
 * not read and out [H uf / df, W uf / df] = sum_l w[l] (the reference's `normalization`).
 * 16-byte accesses when W, kw, sx (scaled) are multiples of 4 and the pointers are 16-byte aligned, element-wise otherwise.
 * Refused (-1, nothing launched): kh > H or kw > W; (H - kh) % sy or (W - kw) % sx != 0 (the reference leaves uncovered pixels: 0 / 0);
 * uf > 1 and df > 1; a non-square window with uf != 1 or df != 1 (get_fold_unfold scales kernel_size[0] on both axes); df not dividing
 * H, W, kh, kw, sy, sx; a window range outside [0, Ly Lx). */
int sdmi_k_patch_unfold(const float* x, const float* c, float* out, int B, int Cx, int Cc, int H, int W, int kh, int kw, int sy, int sx,
                        int l0, int nl, void* stream);
int sdmi_k_patch_fold(const float* o, const float* w, float* out, int B, int C, int H, int W, int kh, int kw, int sy, int sx, int uf, int df,
                      int norm_only, void* stream);
/* SpatialRescaler.forward (modules.py:125-132), method 'bilinear', multiplier 0.5: x fp32 NCHW [B, Cin, H, W] -> out fp32 NCHW
 * [B, Cout, H >> n, W >> n] (w [Cout, Cin], bias [Cout] or NULL), or [B, Cin, H >> n, W >> n] with w == NULL (no channel_mapper).
 * Additive entry points, ABI 17.  The arithmetic is this library's definition:
 *   - one stage: out[i][j] = ((a + b) + (c + d)) * 0.25f with a b at row 2i, cols 2j, 2j+1 and c d at row 2i+1; every stage is rounded
 *     to fp32, no FP contraction.  bilinear at scale 0.5 with align_corners=False samples exactly between two pixels, so an odd last row
 *     or column is never read and the output is H >> n by W >> n.  (torch's CPU kernel sums the four taps in an order that varies with
 *     the shape; the scalings are exact, so the orders differ only in how the sum is rounded.)
 *   - channel map: out[o] = bias[o] + sum_c w[o][c] p[c] in fp32 (fused multiply-add).  Channels go in chunks of 8 round-robin to 8 waves;
 *     a wave sums its channels in ascending order and the 8 wave sums are added to the bias in ascending wave order.  The summation tree
 *     is a function of Cin alone -- never of B, H, W, the load path or the launch geometry; no atomics: two runs give the same bits.
 *   - sdmi_k_spatial_rescale_labels: labels int32 [B, H, W], class c of a pixel = channel c of its one-hot row; x is never built.
 *     p[c] = count_c * 2^(-2n) over the pixel's block for every class in ascending order through the same accumulation code: the output is
 *     bit-identical to sdmi_k_spatial_rescale on one_hot(labels).  A label outside [0, Cin) matches no class (the caller checks the range).
 * 16-byte loads when W % 4 == 0 (n = 2), 8-byte loads when W % 2 == 0 (n = 1), and the pointer is 16-byte aligned; element loads that give
 * the same bits otherwise.  Offsets are 64-bit.
 * Refused (-1, nothing launched): n_stages outside 0 .. 2; Cout outside 1 .. 8 with w set; Cin < 1; B < 1; H or W below 2^n; null x /
 * labels / out; bias without w; the label entry without w. */
int sdmi_k_spatial_rescale(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, int n_stages,
                           int Cout, void* stream);
int sdmi_k_spatial_rescale_labels(const int32_t* labels, const float* w, const float* bias, float* out, int B, int Cin, int H, int W,
                                  int n_stages, int Cout, void* stream);
int sdmi_k_gelu_erf(const float* x, void* out_f16, int64_t n, void* stream);
/* CLIP's quick_gelu, x * sigmoid(1.702 x): fp32 [n] -> fp16 [n], n % 4 == 0 (the mixed text encoder's feed-forward activation) */
int sdmi_k_quick_gelu(const float* x, void* out_f16, int64_t n, void* stream);
/* The two feed-forward activations as producers of a split-fp16 GEMM operand (the full-precision text encoders): fp32 [n], n % 4 == 0
 * -> out = fp16(y), bit for bit what sdmi_k_quick_gelu / sdmi_k_gelu_erf store (y is the same fp32 expression), and out_lo = fp16(y_ref - out):
 * y_ref = y for quick_gelu; for the erf form y_ref = x / 2 erfc(-x / sqrt 2) in fp32, so out + out_lo is the GELU to fp32 accuracy although
 * out keeps the fp16 kernel's bits (its Abramowitz-Stegun erf is up to 2 fp16 ulps off near x = -4; out_lo is then more than half a step of out) */
int sdmi_k_quick_gelu_split(const float* x, void* out, void* out_lo, int64_t n, void* stream);
int sdmi_k_gelu_erf_split(const float* x, void* out, void* out_lo, int64_t n, void* stream);
int sdmi_k_pack_geglu(const float* w, const float* bias, void* wdst_f16, float* bdst, int N, int K, void* stream);
/* Host post-processing of scripts/txt2img.py:313-324, on the device: img fp32 [B, C, H, W] (the
 * decode_first_stage output) -> uint8 [B, H, W, C] = astype(uint8)(255 * clamp((img + 1) / 2, 0, 1)), bit-identical to
 * the reference's torch / numpy ops. */
int sdmi_image_to_uint8(const float* img_nchw, void* out_nhwc_u8, int B, int C, int H, int W, void* stream);
/* fp16 range guard (debug; also SDMI_CHECK_RANGE=1 in the environment): after every launch that writes fp16 activations
 * (MFMA operands: GroupNorm / LayerNorm outputs, q / k / v^T, GEGLU, attention output, fp16 copies of the residual
 * stream) the buffer is scanned.  The reference has the same exposure under torch.autocast (scripts/txt2img.py:283);
 * this makes an overflow visible per launch.  Synchronises the stream after each launch: never on in a timed run.
 * sdmi_range_check(enable) also clears the counters; sdmi_range_report writes
 * {"over_6e4": n, "nonfinite": m, "max_abs": x, "first": "<first offending kernel class>"}. */
int sdmi_range_check(int enable);
int sdmi_range_report(char* json_buf, int json_buf_len);
/* In-situ tuning of the implicit-GEMM tile / split-K choice (no reference counterpart: the reference delegates to
 * MIOpen / hipBLASLt heuristics).  begin -> for r in rounds: sdmi_tune_round(r), run the workloads -> end: every
 * auto-configured GEMM launch between begin and end runs candidate (r mod #candidates) of its shape, timed with HIP
 * events on its stream; end folds the timings into the table and writes it (path NULL = next to libsdmi.so, where it
 * is loaded from at start-up).  sdmi_tune_dump: per-candidate timings of the last collection as text. */
int sdmi_tune_begin(void);
int sdmi_tune_round(int r);
int sdmi_tune_end(const char* path, int* n_keys);
int sdmi_tune_dump(char* buf, int buflen);
/* (tile, split-K) the loaded table holds for a key (host only); kt = K of a conv's 1x1 tail phase: the key that carries it is tried first,
 * then the plain conv's entry (kt = 0; table lines without the optional 12th column).  0 = found, 1 = no entry. */
int sdmi_tune_lookup(int M, int N, int K, int ksize, int stride, int up, int mode, int splitk_req, int kt, int* tile, int* splitk);
/* per-launch timing of the library's kernels (HIP events on the launch stream): begin, run forwards, then end
 * writes a JSON array [{"name","launches","ms","flops","bytes"}] (algorithmic flops / bytes per kernel class) */
int sdmi_profile_begin(void);
int sdmi_profile_end(char* json_buf, int json_buf_len);
/* cache hint used by experiments (tools/bench_prefetch.py): touch every 128-byte line of a device range on `stream` */
int sdmi_k_prefetch_lines(const void* ptr, int64_t bytes, void* stream);
/* a device buffer of >= 256 zero bytes owned by the library (out-of-image conv taps read it) */
const void* sdmi_zero_page(void);

#ifdef __cplusplus
}
#endif
#endif /* SDMI_H_ */

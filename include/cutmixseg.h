/*
 * cutmixseg.h -- C ABI of libcutmixseg_hip.so: the MI355X (gfx950) kernels behind the CutMix mean-teacher training
 * step of Britefury/cutmix-semisup-seg (train_seg_semisup_mask_mt.py).
 *
 * The reference has no FFI: its boundary is the Python API. Each entry point below names the
 * reference code (file:line, relative to the upstream repository root) whose device work it replaces; the Python
 * mirror of the reference interface (cutmix-semisup-seg_amd/) binds these with ctypes -- see INTEGRATION.md for
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless its name ends in `_host`
 *   - the caller owns every buffer; the library allocates nothing, never synchronises and enqueues all work on
 *     `stream` (a hipStream_t passed as void*); calls are capturable in a hipGraph
 *   - tensors are dense NCHW unless stated otherwise
 *   - returns 0 on success or a negative CMS_E* code; never throws; cms_last_error() gives a thread-local message
 *   - `dtype` arguments: CMS_F32 or CMS_BF16
 *   - low-resolution logits + (H, W, align_corners) describe an implicit bilinear upsample that is evaluated inside
 *     the kernel (full-resolution logits are never materialised); pass h == H and w == W for plain logits
 */
#ifndef CUTMIXSEG_H
#define CUTMIXSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMS_VERSION 101

#define CMS_OK 0
#define CMS_EINVAL (-1)     /* bad argument */
#define CMS_ELAUNCH (-2)    /* kernel launch / HIP runtime error */
#define CMS_EUNSUPPORTED (-3)

#define CMS_F32 0
#define CMS_BF16 1

#define CMS_LABEL_U8 0
#define CMS_LABEL_I64 1

/* cons_loss_fn, train_seg_semisup_mask_mt.py:428-446 */
#define CMS_LOSS_VAR 0
#define CMS_LOSS_LOGITS_VAR 1
#define CMS_LOSS_LOGITS_SMOOTHL1 2
#define CMS_LOSS_BCE 3
#define CMS_LOSS_KLD 4

/* mask_mode, train_seg_semisup_mask_mt.py:27-33 */
#define CMS_MODE_MIX 0
#define CMS_MODE_CUT 1

int cms_version(void);
const char* cms_last_error(void);
/* number of compute units / name of the current device (device-props cache) */
int cms_device_info(int* n_cu, char* name_out, size_t name_cap);

/* ------------------------------------------------------------------------------------------------------------
 * Box masks + CutMix paste      (mask_gen.py:110-120 ; train_seg_semisup_mask_mt.py:346-351, 363, 385-389)
 *
 * `ranges`: int32 (N, n_boxes, 4) = [y0, y1, x0, x1] half-open, i.e. the reference's float rectangles after its
 * `int(y0):int(y1)` slicing rules (done on the host by the Python side). Boxes XOR; `invert` != 0 means box = 1.
 * ------------------------------------------------------------------------------------------------------------ */

/* mask_out f32 (N,1,H,W): what BoxMaskGenerator.generate_params returns / torch_masks_from_params passes through */
int cms_boxmask_rasterize(const int32_t* ranges, int n, int n_boxes, int h, int w, int invert,
                          float* mask_out, void* stream);

/* out[n,c,y,x] = m ? x1 : x0, with m rasterised in-kernel from `ranges` (mask never touches HBM).
 * x0 == NULL means zeros (cut mode: x * m, :389). Exact for m in {0,1} (x0*(1-m) + x1*m, :350). */
int cms_cutmix_paste(const void* x0, const void* x1, void* out, int dtype, const int32_t* ranges, int n,
                     int n_boxes, int c, int h, int w, int invert, void* stream);

/* same with a materialised f32 mask (N,1,H,W), computed arithmetically as x0*(1-m) + x1*m (any mask values) */
int cms_cutmix_paste_mask(const void* x0, const void* x1, void* out, int dtype, const float* mask, int n, int c,
                          int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Masked consistency loss, fused: bilinear upsample + teacher-logit paste + softmax + confidence + loss
 *                               (train_seg_semisup_mask_mt.py:363-367, 407-459)
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct cms_consistency_desc {
    const float* l_stu;    /* (N,C,h,w) student logits (of the pasted / cut image)                          */
    const float* l_tea0;   /* (N,C,h,w) teacher logits of image 0                                            */
    const float* l_tea1;   /* (N,C,h,w) teacher logits of image 1 (mix mode) or NULL (cut mode)              */
    const int32_t* ranges; /* (N,n_boxes,4) box ranges, or NULL when `mask` is given                         */
    const float* mask;     /* (N,1,H,W) materialised box mask, or NULL when `ranges` is given                */
    const float* um0;      /* (N,1,H,W) validity mask of image 0, NULL = all ones                            */
    const float* um1;      /* (N,1,H,W) validity mask of image 1, NULL = all ones (ignored in cut mode)      */
    int n, c, h, w;        /* logits geometry                                                                */
    int H, W;              /* loss geometry (crop size); logits are upsampled h x w -> H x W in-kernel       */
    int align_corners;     /* 1: deeplab2.py:204 ; 0: deeplab3plus.py:77                                     */
    int n_boxes, invert;
    int mode;              /* CMS_MODE_MIX / CMS_MODE_CUT                                                    */
    int loss_fn;           /* CMS_LOSS_*                                                                     */
    float conf_thresh;     /* <= 0 disables confidence thresholding (:408)                                   */
    int conf_per_pixel;    /* --conf_per_pixel (:415)                                                        */
} cms_consistency_desc;

/* bytes of scratch needed by cms_consistency_fwd (per-workgroup partial sums) */
size_t cms_consistency_workspace_bytes(const cms_consistency_desc* d);

/* stats_out: double[4] = { sum(loss*um), sum(loss*um*conf), count(conf >= thresh), P = N*H*W } (device).
 * Deterministic (fixed-order second-stage reduction). Under data parallelism the caller all-reduces
 * stats[2..3] before cms_consistency_finalize. */
int cms_consistency_fwd(const cms_consistency_desc* d, void* workspace, double* stats_out, void* stream);

/* scalars_out: float[4] = { consistency_loss (the value the reference logs, :461), conf_rate (:413, NaN if
 * disabled), grad_scale (d unsup_loss / d per-pixel masked loss), unsup_loss (:458) } (device).
 * `stats_global` = stats used for the confidence rate (== stats_local on one GPU). No host sync. */
int cms_consistency_finalize(const double* stats_local, const double* stats_global, float conf_thresh,
                             int conf_per_pixel, float ramp_val, float cons_weight, float* scalars_out,
                             void* stream);

/* grad_l_stu f32 (N,C,h,w) += d unsup_loss / d l_stu (caller zero-fills when it wants `=`); reads scalars[2] */
int cms_consistency_bwd(const cms_consistency_desc* d, const float* scalars, float* grad_l_stu, void* stream);

/* (round 6) Forward AND backward in one launch (train_seg_semisup_mask_mt.py:363-367, 407-459 and their autograd twins). The
 * backward pass needs ONE scalar of the forward pass -- the confidence rate of the default mode (:415-418) -- and is linear in
 * it: this launch writes stats_out (as cms_consistency_fwd) and ADDS to grad_l_stu the gradient with that scalar left out,
 *     grad_unit * um * [conf >= thresh, --conf_per_pixel only] * d per-pixel loss / d l_stu,   grad_unit = ramp * weight / (N*H*W);
 * behind cms_consistency_finalize the caller multiplies the rows by the rate (default mode with a threshold only):
 *     cms_scale_by_scalar(grad_l_stu, n*c*h*w, scalars, 1, 1.0f, stream).
 * So grad_l_stu must hold nothing else yet (zero-filled rows). cms_consistency_fused_supported: 1 when the launch exists for
 * the descriptor (an upsampling geometry whose tile rectangles fit the LDS, not the deterministic mode); the workspace is
 * cms_consistency_workspace_bytes as before. CMS_LOSS_FUSED=0 in the environment switches both fused launches off. */
int cms_consistency_fused_supported(const cms_consistency_desc* d);
int cms_consistency_fwd_bwd(const cms_consistency_desc* d, float grad_unit, void* workspace, double* stats_out,
                            float* grad_l_stu, void* stream);
/* x[i] *= scalars[index] * factor, i < n: the deferred scalar factor of the fused loss launches (a device scalar, no host sync) */
int cms_scale_by_scalar(float* x, long long n, const float* scalars, int index, float factor, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Class-threshold consistency: the masked consistency loss above with a per-class confidence threshold, and the
 * statistics a self-adaptive threshold (FreeMatch, Wang et al., ICLR 2023) is made from riding in the loss launch.
 * The project's own definition. For a pixel of a call, with t its pasted, bilinearly upsampled teacher logit row:
 *   m = max t, z = sum_k exp(t_k - m), conf = 1 / z   (the very float compared with conf_thresh above)
 *   k*  = the smallest index with t_k == m;   q_c = exp(t_c - m) / z
 *   pass bit = conf >= thr[k*] in fp32 (a NaN fails). It takes the place of `conf >= conf_thresh` everywhere: in the
 *   count behind the rate of the default mode (sum of bits / P over all pixels) and as the factor of conf_per_pixel.
 *   cons.conf_thresh is not read: the threshold is always on. Loss sums, cms_consistency_finalize (call it with any
 *   conf_thresh > 0), cms_scale_by_scalar and the deferred-rate contract of cms_consistency_fwd_bwd are unchanged.
 *   valid pixel (statistics only): mix -- the validity map of the image the mask selects is >= 0.5; cut -- um0 >= 0.5
 *   whatever the mask bit (the prediction is image 0's everywhere); a missing map is all valid.
 * cms_cthresh_fwd and cms_cthresh_fwd_bwd ADD into `table`, unsigned 64-bit integers (no sum depends on the order of
 * additions, or on how a batch is split into calls). The buffer holds CMS_CTHRESH_REPLICAS copies of the layout below, one
 * after the other; a workgroup adds into copy (its index mod CMS_CTHRESH_REPLICAS), so that the workgroups of a launch do not
 * all queue at the same 2 + 3C addresses, and THE table is the sum of the copies (cms_cthresh_update reads it so):
 *   table[0] = n_valid, table[1] = S_conf = sum_valid rint(conf * 2^24), table[2 + c] = S_c = sum_valid rint(q_c * 2^24),
 *   table[2 + C + c] = N_pred[c] = valid pixels with k* == c, table[2 + 2C + c] = N_pass[c] = those of them that pass.
 *   (A NaN contributes 0 to S_conf / S_c.) cms_cthresh_bwd reads thr only. At most 128 classes.
 * Geometry routes, workspace, stats_out, scalars, grad_unit and error codes are those of the cms_consistency_* twins.
 * ------------------------------------------------------------------------------------------------------------ */
#define CMS_CTHRESH_REPLICAS 32
typedef struct cms_cthresh_desc {
    cms_consistency_desc cons;      /* as above; conf_thresh is not read                                      */
    const float* thr;               /* f32[C] per-class thresholds (device)                                   */
    unsigned long long* table;      /* u64[CMS_CTHRESH_REPLICAS][2 + 3C] statistics of the iteration (device), added into */
} cms_cthresh_desc;
size_t cms_cthresh_workspace_bytes(const cms_cthresh_desc* d);
int cms_cthresh_fused_supported(const cms_cthresh_desc* d);
int cms_cthresh_fwd(const cms_cthresh_desc* d, void* workspace, double* stats_out, void* stream);
int cms_cthresh_bwd(const cms_cthresh_desc* d, const float* scalars, float* grad_l_stu, void* stream);
int cms_cthresh_fwd_bwd(const cms_cthresh_desc* d, float grad_unit, void* workspace, double* stats_out, float* grad_l_stu,
                        void* stream);
/* One launch, one thread, fp64: folds the iteration's table. state = f64[1 + C] = { tau, p~_c }; epoch = u64[1 + 2C] =
 * { n_valid, N_pred[c], N_pass[c] }. adaptive != 0 and n_valid > 0:
 *   mu = S_conf / (2^24 n_valid), pi_c = S_c / (2^24 n_valid); tau <- ema tau + (1 - ema) mu; p~_c <- ema p~_c + (1 - ema) pi_c;
 *   thr_c = fp32(min(ceil, max(floor, tau * p~_c / max_j p~_j))).
 * Always: n_valid, N_pred and N_pass are added into `epoch` and the table (every copy) is zeroed. The caller starts from
 * tau = p~_c = 1 / C and thr_c = clamp(1 / C), and runs this ahead of an iteration's loss launches: the thresholds an
 * iteration applies are made from the iterations before it (one iteration behind the paper's update-then-mask, so that
 * the sums ride in the loss launch and thr is constant within a step). The paper's fairness loss is not built. */
int cms_cthresh_update(int n_classes, int adaptive, double ema, double floor_v, double ceil_v, double* state, float* thr,
                       unsigned long long* table, unsigned long long* epoch, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Supervised cross entropy, fused: bilinear upsample + log-softmax + NLL(ignore_index)
 *                               (nn.CrossEntropyLoss(ignore_index=255), train_seg_semisup_mask_mt.py:126, 299-301)
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct cms_ce_desc {
    const float* logits;  /* (N,C,h,w) */
    const void* labels;   /* (N,H,W) uint8 or int64 */
    int label_dtype;      /* CMS_LABEL_U8 / CMS_LABEL_I64 */
    int ignore_index;
    int n, c, h, w, H, W, align_corners;
} cms_ce_desc;

size_t cms_ce_workspace_bytes(const cms_ce_desc* d);
/* stats_out: double[2] = { sum over valid pixels of -log p[label], number of valid pixels } */
int cms_ce_fwd(const cms_ce_desc* d, void* workspace, double* stats_out, void* stream);
/* scalars_out: float[2] = { loss = sum / count, grad_scale = loss_weight / count } from (possibly all-reduced)
 * stats */
int cms_ce_finalize(const double* stats, float loss_weight, float* scalars_out, void* stream);
int cms_ce_bwd(const cms_ce_desc* d, const float* scalars, float* grad_logits, void* stream);
/* (round 6) forward AND backward in one launch (autograd of :126, 299-301): stats_out as cms_ce_fwd; grad_logits += (softmax -
 * onehot) of every valid pixel through the adjoint of the upsample, WITHOUT the factor loss_weight / count -- behind
 * cms_ce_finalize: cms_scale_by_scalar(grad_logits, n*c*h*w, scalars, 1, 1.0f, stream). Rows must be zero on entry. */
int cms_ce_fused_supported(const cms_ce_desc* d);
int cms_ce_fwd_bwd(const cms_ce_desc* d, void* workspace, double* stats_out, float* grad_logits, void* stream);
/* The backward kernels of both losses scatter through tiles that share low-resolution cells with their neighbours. on = 1:
 * the tiles are issued as colour classes that never share a cell (four launches, run-to-run reproducible gradients -- what
 * `--deterministic` asks for); 0 (default; CMS_LOSS_DETERMINISTIC=1 in the environment flips it): one launch, fp32 atomics in a
 * run-dependent order (~1e-7), like the weight gradients' default. */
int cms_loss_set_deterministic(int on);

/* ------------------------------------------------------------------------------------------------------------
 * ICT (interpolation consistency training): per-sample blends and the fused interpolation loss
 *                               (train_seg_semisup_ict.py:306-391)
 * ------------------------------------------------------------------------------------------------------------ */

/* out[i, :] = x0[i, :] * (1 - lam[i]) + x1[i, :] * lam[i] for n samples of `chw` elements each (:310-311). fp32 arithmetic in
 * the reference's order (1 - lam in fp32, two rounded products, their sum; no FMA), one rounding to bf16 for CMS_BF16. `lam`:
 * n device floats. Images (chw = C*H*W) and, with CMS_F32 and chw = H*W, validity masks. 16-byte accesses when the three
 * pointers are 16-byte aligned, element-wise otherwise. */
int cms_ict_blend(const void* x0, const void* x1, void* out, int dtype, const float* lam, int n, long long chw, void* stream);

/* The loss: the teacher's two predictions are BLENDED per sample, probabilities p_t = softmax(L0)(1-lam) + softmax(L1) lam for
 * var / bce / kld, logits l_t = L0 (1-lam) + L1 lam for logits_var / logits_smoothl1 (:328-329, 360-380); the confidence is
 * max softmax(L0) (1-lam) + max softmax(L1) lam (:338-341); the loss mask is um0 (1-lam) + um1 lam (:311), blended in-kernel. */
typedef struct cms_ict_desc {
    const float* l_stu;    /* (N,C,h,w) student logits of the blended image                                  */
    const float* l_tea0;   /* (N,C,h,w) teacher logits of image 0                                            */
    const float* l_tea1;   /* (N,C,h,w) teacher logits of image 1                                            */
    const float* lam;      /* (N) mix factors                                                                */
    const float* um0;      /* (N,1,H,W) validity mask of image 0, NULL = all ones                            */
    const float* um1;      /* (N,1,H,W) validity mask of image 1, NULL = all ones                            */
    int n, c, h, w;        /* logits geometry                                                                */
    int H, W;              /* loss geometry (crop size); logits are upsampled h x w -> H x W in-kernel       */
    int align_corners;
    int loss_fn;           /* CMS_LOSS_*                                                                     */
    float conf_thresh;     /* <= 0 disables confidence thresholding (:334)                                   */
    int conf_per_pixel;    /* --conf_per_pixel (:347), with the reference's broadcast: see below             */
} cms_ict_desc;

/* bytes of scratch for cms_ict_fwd / cms_ict_bwd: per-workgroup partial sums and, with conf_per_pixel and a threshold, the
 * (H,W) map of sum_i [conf(i,y,x) >= thresh] */
size_t cms_ict_workspace_bytes(const cms_ict_desc* d);

/* stats_out: double[4] = { sum(loss*um), sum(loss*um*cbar), count(conf >= thresh), P = N*H*W } (device), the contract of
 * cms_consistency_fwd, so cms_consistency_finalize turns it into the loss, the rate and the gradient scale unchanged.
 * --conf_per_pixel: the reference's mask comes out as (N,1,1,H,W) against a (N,1,H,W) loss (:343 indexes a keepdim tensor), and
 * the mean over the (N,N,1,H,W) product weights pixel (y,x) of EVERY sample with cbar[y,x] = (1/N) sum_i [conf(i,y,x) >=
 * thresh], the batch mean of the indicator: a first launch writes the map of that sum into `workspace`, the loss launch and
 * cms_ict_bwd read it. The workspace is the caller's and must stay intact between cms_ict_fwd and cms_ict_bwd. Without
 * conf_per_pixel no map is written and stats_out[1] holds sum(loss*um*[own conf >= thresh]), which nothing reads. */
int cms_ict_fwd(const cms_ict_desc* d, void* workspace, double* stats_out, void* stream);

/* grad_l_stu f32 (N,C,h,w) += d unsup_loss / d l_stu; reads scalars[2] (cms_consistency_finalize) and, with conf_per_pixel,
 * the map cms_ict_fwd left in `workspace`. cms_loss_set_deterministic applies. */
int cms_ict_bwd(const cms_ict_desc* d, const void* workspace, const float* scalars, float* grad_l_stu, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Augmentation consistency (the classic mean teacher between two augmented views): the fused affine-warp loss
 *                               (train_seg_semisup_aug_mt.py:302-390)
 * ------------------------------------------------------------------------------------------------------------ */

/* The teacher's prediction of view 0 is warped into the student's view 1 per pixel: a student pixel (x, y) samples the teacher's
 * full-resolution map at ix = a00 x + a01 y + a02, iy = a10 x + a11 y + a12 with the four taps and the zero padding of
 * F.grid_sample(bilinear). `xf` holds these PIXEL-space matrices, one per sample: F.affine_grid(theta, align_corners=True)
 * followed by grid_sample's un-normalisation, folded:  a00 = t00, a01 = t01 (W-1)/(H-1), a02 = (t02 - t00 - t01 + 1)(W-1)/2,
 * a10 = t10 (H-1)/(W-1), a11 = t11, a12 = (t12 - t10 - t11 + 1)(H-1)/2. Only that grid convention is supported (the reference
 * passes no other). The target is sum_k w_k softmax(L_k) for var / bce / kld and sum_k w_k L_k for logits_var /
 * logits_smoothl1, L_k = the teacher's logits at tap k (the bilinear upsample of l_tea, as the network's own); the confidence
 * is the max of the warped probabilities (:347); the loss mask is grid_sample(um0) * um1 (:306). No full-resolution map is
 * written. logits_var: sum_c (delta logits)^2 / sqrt(C) -- the reference's branch raises, this is its evident intent. */
typedef struct cms_aug_desc {
    const float* l_stu;    /* (N,C,h,w) student logits of view 1                                              */
    const float* l_tea;    /* (N,C,h,w) teacher logits of view 0                                              */
    const float* xf;       /* (N,6) pixel-space warp matrices, view-1 pixel -> view-0 position (device)       */
    const float* um0;      /* (N,1,H,W) validity mask of view 0, NULL = all ones (still zero-padded)          */
    const float* um1;      /* (N,1,H,W) validity mask of view 1, NULL = all ones                              */
    int n, c, h, w;        /* logits geometry                                                                 */
    int H, W;              /* loss geometry (crop size), H >= 2 and W >= 2                                    */
    int align_corners;     /* of the networks' upsample h x w -> H x W                                        */
    int loss_fn;           /* CMS_LOSS_*                                                                      */
    float conf_thresh;     /* <= 0 disables confidence thresholding (:345)                                    */
    int conf_per_pixel;    /* --conf_per_pixel (:353): (N,1,H,W) against (N,1,H,W), the pixel's own indicator */
    int force_global;      /* != 0: never stage the teacher's rectangle in LDS (same results bit for bit)     */
} cms_aug_desc;

/* bytes of scratch for cms_aug_fwd: per-workgroup partial sums */
size_t cms_aug_workspace_bytes(const cms_aug_desc* d);

/* stats_out: double[4] = { sum(loss*mask), sum(loss*mask*[conf >= thresh]), count(conf >= thresh), P = N*H*W } (device), the
 * contract of cms_consistency_fwd: cms_consistency_finalize turns it into the loss, the rate and the gradient scale unchanged. */
int cms_aug_fwd(const cms_aug_desc* d, void* workspace, double* stats_out, void* stream);

/* grad_l_stu f32 (N,C,h,w) += d unsup_loss / d l_stu; reads scalars[2] (cms_consistency_finalize). The teacher carries no
 * gradient. cms_loss_set_deterministic applies. */
int cms_aug_bwd(const cms_aug_desc* d, const float* scalars, float* grad_l_stu, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Bilinear upsample (F.interpolate(mode='bilinear'), architectures/deeplab2.py:204, deeplab3plus.py:54-55,77)
 * Stand-alone form for the `forward(x) -> (N,C,H,W)` contract of the reference models.
 * ------------------------------------------------------------------------------------------------------------ */
int cms_upsample_bilinear_fwd(const float* lo, float* hi, int n, int c, int h, int w, int H, int W,
                              int align_corners, void* stream);
/* grad_lo (N,C,h,w) = adjoint applied to grad_hi (overwrites); deterministic gather */
int cms_upsample_bilinear_bwd(const float* grad_hi, float* grad_lo, int n, int c, int h, int w, int H, int W,
                              int align_corners, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Teacher EMA and fused optimizer + EMA over flat fp32 arenas
 *                               (optim_weight_ema.py:21-25 ; torch.optim.Adam/SGD at
 *                                train_seg_semisup_mask_mt.py:90-100, 465-467)
 * ------------------------------------------------------------------------------------------------------------ */

/* tgt = tgt*alpha + src*one_minus_alpha with the reference's three fp32 roundings (no FMA). Optional bf16 copy
 * of the new target. */
int cms_ema_flat(float* tgt, const float* src, size_t count, float alpha, float one_minus_alpha,
                 uint16_t* tgt_bf16_out, void* stream);

/* One segment of the parameter arena (a state_dict tensor). `k_updates` = how many times the tensor appears in
 * the optimizer's parameter list (deeplab2.py:208-230 yields backbone weights 3x/4x): the update is applied k
 * times in sequence with the same gradient; 0 = not optimised (BN tensors, or tensors that never receive a
 * gradient such as the ASPP d18/d24 branches) -> only the EMA is applied. */
typedef struct cms_param_segment {
    uint64_t offset;     /* first element in the arenas */
    uint64_t count;      /* number of elements */
    int32_t k_updates;
    int32_t lr_group;    /* index into the `lrs` array */
} cms_param_segment;

typedef struct cms_optim_desc {
    float* param;              /* student fp32 master arena */
    const float* grad;         /* gradient arena (same indexing) */
    float* slot0;              /* Adam exp_avg / SGD momentum buffer */
    float* slot1;              /* Adam exp_avg_sq (unused for SGD) */
    float* ema_param;          /* teacher fp32 arena, or NULL (pi model) */
    uint16_t* param_bf16;      /* optional bf16 copy of the updated student arena */
    uint16_t* ema_bf16;        /* optional bf16 copy of the updated teacher arena */
    const cms_param_segment* segments; /* DEVICE array */
    const uint32_t* chunk_seg; /* DEVICE array: segment index of every CMS_OPT_CHUNK-element chunk of work */
    const uint32_t* chunk_off; /* DEVICE array: element offset of the chunk inside its segment */
    uint32_t n_chunks;
    const double* lrs;         /* DEVICE array: current learning rate per group (double, as Python holds it) */
    const int64_t* step_count; /* DEVICE scalar: number of optimizer steps already taken */
    float grad_scale;          /* gradients are multiplied by this first (1/world_size after a sum all-reduce) */
    float ema_alpha;
    float ema_one_minus_alpha; /* (float)(1.0 - (double)alpha), as the reference forms it */
    /* Adam (doubles: torch forms 1-beta and the bias corrections in Python double before the fp32 ops) */
    double beta1, beta2, eps;
    /* SGD */
    float momentum, weight_decay;
    int nesterov;
} cms_optim_desc;

#define CMS_OPT_CHUNK 2048

int cms_adam_ema_step(const cms_optim_desc* d, void* stream);
int cms_sgd_ema_step(const cms_optim_desc* d, void* stream);
/* *counter += 1 on the device (keeps the optimizer step counter graph-replayable) */
int cms_increment_counter(int64_t* counter, void* stream);
/* Frozen BatchNorm of ALL layers of a network folded into the convolution epilogues' affine in one launch
 * (architectures/deeplab2.py:92-107, BatchNorm in eval mode: y = (x - mean) / sqrt(var + eps) * weight + bias):
 *   scale[i] = flat[idx_weight[i]] * rsqrt(flat[idx_var[i]] + eps),  bias[i] = flat[idx_bias[i]] - flat[idx_mean[i]] * scale[i]
 * `flat`: the fp32 parameter arena; idx_*: n element indices into it (int64, device); every product / difference rounded
 * separately, like the tensor expression of the reference's modules. */
int cms_bn_fold(const float* flat, const int64_t* idx_weight, const int64_t* idx_bias, const int64_t* idx_mean,
                const int64_t* idx_var, int n, float eps, float* scale, float* bias, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation: fused upsample + argmax + confusion matrix   (train_seg_semisup_mask_mt.py:510-514 ; evaluation.py)
 * I = diag(cm), U = rowsum + colsum - diag so one CxC histogram is all that is needed.
 * ------------------------------------------------------------------------------------------------------------ */
/* cm int64 (C,C) += histogram of (truth, argmax) over pixels with truth != ignore_index (ignore_index < 0: none).
 * pred_out (N,H,W) uint8 optional. */
int cms_argmax_confusion(const float* logits, const void* labels, int label_dtype, int ignore_index, int n, int c,
                         int h, int w, int H, int W, int align_corners, int64_t* cm, uint8_t* pred_out,
                         void* stream);
/* fast_cm / per_class_i_and_u_cm on integer maps (evaluation.py:6-37): truth, pred uint8 (count) */
int cms_confusion(const uint8_t* truth, const uint8_t* pred, size_t count, int ignore_index, int c, int64_t* cm,
                  void* stream);
/* Hole filling of binary predictions on the device (evaluation.py:53-55: scipy.ndimage.binary_fill_holes(pred != 0), default
 * structure, bit-identical): pred (n,h,w) uint8, 0 = background, anything else foreground. A background pixel is kept iff it is
 * 4-connected through background pixels to the outside of its image (every background pixel on the first / last row or column
 * touches the outside); every other pixel comes out as 1. Each of the n images is filled on its own. Three stream-ordered
 * launches (tile-local union-find, seams, resolve), no host synchronisation.
 *   out    (n,h,w) uint8 in {0,1}; may alias pred; may be NULL when only cm is wanted
 *   truth  (n,h,w) uint8 and cm int64 (2,2): both NULL or both given; cm[truth][filled] += counts over pixels with
 *          truth != ignore_index (ignore_index < 0: none) and truth < 2, as cms_confusion would on the filled map
 *   workspace: cms_fill_holes_workspace_bytes(n, h, w) bytes of device memory (one int32 per pixel plus one per image);
 *          that function returns 0 for non-positive geometry or n * (h * w + 1) >= 2^31, which cms_fill_holes refuses */
size_t cms_fill_holes_workspace_bytes(int n, int h, int w);
int cms_fill_holes(const uint8_t* pred, uint8_t* out, const uint8_t* truth, int ignore_index, int64_t* cm, int n, int h, int w,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * MFMA implicit-GEMM convolution for the backbone   (nn.Conv2d + frozen nn.BatchNorm2d + ReLU (+ residual) of
 *                               architectures/deeplab2.py:89-109, 124-128, and their backward passes)
 * Activations bf16 NHWC, weights bf16 [tap][Cout][Cin], fp32 accumulation.
 * ------------------------------------------------------------------------------------------------------------ */
#define CMS_CONV_MAX_TAPS 18
#define CMS_CONV_FWD 0     /* y  = relu(acc * scale[co] + bias[co] + res)                     */
#define CMS_CONV_DGRAD 1   /* dx = (acc + res) * [mask_src > 0]                               */

typedef struct cms_conv_desc {
    const void* x;         /* bf16 [N][H][W][Cin]                                                                */
    const void* w;         /* bf16 [ntaps][Cout][Cin]                                                            */
    void* y;               /* bf16 [N][out_h][out_w][Cout] or NULL                                               */
    float* y32;            /* fp32 NCHW [N][cout_real][Ho][Wo] or NULL (ASPP head logits)                         */
    const float* scale;    /* [Cout] or NULL: frozen-BN gamma/sqrt(var+eps)                                       */
    const float* bias;     /* [Cout] or NULL: frozen-BN beta - mean*scale, or the conv bias                       */
    const void* res;       /* bf16, indexed like y: residual (forward) / gradient to add (dgrad), or NULL         */
    const void* mask_src;  /* bf16, indexed like y: dgrad output is zeroed where this activation is <= 0, or NULL */
    int n, h, w_in, cin;   /* input geometry                                                                     */
    int ho, wo, cout;      /* GEMM pixel grid (N*ho*wo rows) and channel count (multiple of 32)                   */
    int cout_real;         /* channels actually written to y32 (<= cout); must equal cout for the bf16 output     */
    int ntaps;             /* kernel taps; tap t reads input pixel (oy*stride + tap_dy[t], ox*stride + tap_dx[t]) */
    int tap_dy[CMS_CONV_MAX_TAPS], tap_dx[CMS_CONV_MAX_TAPS];
    int stride;            /* input gather stride                                                                */
    int out_h, out_w, out_stride; /* output tensor geometry; pixel (oy,ox) is written at (oy*out_stride, ...)      */
    int relu;              /* forward epilogue ReLU                                                              */
    int mode;              /* CMS_CONV_FWD / CMS_CONV_DGRAD                                                      */
    int tile;              /* 0 = auto, else channels per workgroup: 128 / 64 / 32                               */
    int ksplit;            /* <= 1: off; else the taps are split over workgroups (fp32 y32 output only, which must
                              be zero-filled: partial sums are accumulated with atomics; bias added once)        */
    const void* zeros;     /* a run of zero bytes in device memory, at least 2 * cin + 128 long: enables the
                              direct-to-LDS loader (padded / out-of-range rows are fetched from it, advancing through
                              it like a live pixel's channel run); NULL = register-staged loader                 */
    int variant;           /* 0 = auto (direct-to-LDS, buffer-addressed below 2 GB per tensor, flat addresses above),
                              1 = register-staged loader, 30 = variant 0 with cycle stamps (cms_conv_set_trace), 43 = the
                              flat-address direct-to-LDS loader at any size; 90 = the eight-phase 256 x 256 kernel, one
                              whole tile per workgroup; 92 = 90 with cycle stamps; 99 = never the eight-phase kernel.
                              Any other code is an error (the stage rings, two-stage loaders, K rotation, ablation
                              switches and the persistent stream-K launch 91 / 93 that once had codes were measured,
                              none faster, and removed: DESIGN.md section 4.1, docs/DESIGN_HISTORY.md 4.4)        */
    int zeros_bytes;       /* length of the `zeros` run (checked against 2 * cin + 128)                          */
    /* ReLU masks as BITS (round 4). A forward launch with `relu` can also write, per output pixel, Cout / 8 bytes whose bit
     * c & 7 of byte c >> 3 says [y[pixel][c] > 0] (of the stored bf16 value): mask_bits_out = uint8 [N][out_h][out_w][cout / 8].
     * The data gradient that would re-read that activation only for its sign (`mask_src`) takes the bits instead
     * (`mask_bits`, mask_src NULL): 1/16 of the bytes -- 69 MB less per layer-3 expansion of BASELINE configs[1] -- and the same
     * result bit for bit. Both kernels of cms_conv_igemm write and read the same layout (round 5: the eight-phase kernel too,
     * whole-tile launches).                                                                                                  */
    uint8_t* mask_bits_out;
    const uint8_t* mask_bits;
    /* Round 5: BatchNorm statistics out of the convolution epilogue (the batch-statistics units of
     * architectures/deeplab2.py:72-84 -- the reference CLI's default, train_seg_semisup_mask_mt.py:587 -- are
     * u = conv(x); y = relu(bn_batch(u) (+ res)): the statistics pass over u, one of the unit's memory passes, disappears).
     * stats_out != NULL (bf16 NHWC output, mode 0): every workgroup also writes the per-channel (sum, sum of squares) of the bf16
     * values it STORES, per pixel tile: float [tiles][2 slots][2][cout], tiles = ceil(n * ho * wo / T), T =
     * cms_conv_igemm_stats_tile_rows(desc) (128 or 256 rows: the kernel that runs the launch; 0 = this launch cannot, use
     * CMS_BN_STATS). The pixel rows are `groups` equal runs of stats_rows_per_group rows (sample groups normalised separately);
     * slot 0 = the tile's rows of the group its FIRST row belongs to, slot 1 = its rows of the next group (written only by a tile that
     * straddles a boundary). CMS_BN_FINALIZE_TILES turns them into mean / rstd / scale / shift and moves the running statistics. */
    float* stats_out;
    int stats_rows_per_group;
    /* Round 5, data gradients with BOTH res and mask_bits: != 0 -> the bits gate the residual only, y = acc + (bit ? res : 0)
     * (the masked gradient of an identity shortcut added to a convolution's data gradient: the batch-statistics bottleneck's
     * `dres` tensor is never written, architectures/deeplab2.py:105-107); 0 -> y = bit ? acc + res : 0 as before.           */
    int mask_gates_res;
    /* Round 5, data gradients (mode 1) with stats_out: the launch writes the gradient dy of the OUTPUT of a batch-statistics unit
     * y = relu(bn(u) (+ res)); with that unit's u (bf16, indexed like this launch's output), ReLU mask bits (NULL: no ReLU) and
     * statistics mean / rstd [groups][cout] it also leaves per-tile (sum d, sum d * xhat), d = bit ? dy : 0, xhat = (u - mean) * rstd --
     * CMS_BN_BWD_SUMS_TILES adds them into the sums CMS_BN_BWD_APPLY takes: the unit's backward reduction over u, dy and the
     * mask (CMS_BN_REDUCE_BWD) is not launched. The stored output is unchanged (unmasked dy).                              */
    const void* bstats_u;
    const uint8_t* bstats_bits;
    const float* bstats_mean;
    const float* bstats_rstd;
} cms_conv_desc;

int cms_conv_igemm(const cms_conv_desc* d, void* stream);
/* Which kernel cms_conv_igemm runs this descriptor on (measurement tooling: algorithmic bytes per KERNEL beside the PMC
 * counters; the choice depends on the geometry and on the CMS_CONV8 switch of the process). */
#define CMS_ROUTE_OTHER 0     /* an explicit variant / tile request */
#define CMS_ROUTE_TILE128 1   /* conv_igemm_kernel, 128 channels x 128 pixels */
#define CMS_ROUTE_MIXED 2     /* conv_igemm_mixed_kernel: the balanced 128 x 128 launch */
#define CMS_ROUTE_TILE64 3    /* 64-channel tile */
#define CMS_ROUTE_TILE32 4    /* 32-channel tile */
#define CMS_ROUTE_CONV8 8     /* conv8_kernel: eight-phase 256 x 256 */
int cms_conv_igemm_route(const cms_conv_desc* d);
/* pixel rows per statistics tile of a launch with stats_out (see cms_conv_desc), or 0 when the launch cannot write them */
int cms_conv_igemm_stats_tile_rows(const cms_conv_desc* d);

/* Diagnostic (tools/conv_trace.py): launches with variant 30 stamp s_memtime at every phase of the K loop of wave 0
 * (own loads landed / barrier / MFMAs issued / barrier / next stage issued) into `buf`: 512 dwords per workgroup for
 * the first `workgroups` workgroups -- dwords 0..12 = HW_ID, XCC_ID, s_memrealtime at start (lo, hi), cycles since
 * start at: prologue done, K loop done, epilogue arithmetic done, stores acknowledged; K steps; tile_m; tile_n;
 * s_memtime at start (lo, hi); from dword 16 on six stamps per K step. While a buffer is set, cms_conv_wgrad launches
 * stamp their stages the same way (tools/wgrad_trace.py). NULL switches it off. Not part of the data path. */
int cms_conv_set_trace(void* buf, int workgroups);

/* dst[tap'][ci][co] = bf16(src[tap][co][ci] * scale[co]) with tap' = ntaps-1-tap when flip != 0: the operand of
 * the dgrad pass (which is cms_conv_igemm on the transposed, tap-flipped, BN-scale-folded weights). */
int cms_conv_pack_transpose(const void* src, int src_dtype, void* dst_bf16, const float* scale, int ntaps, int cout,
                            int cin, int flip, void* stream);

/* The same for many weight tensors in ONE launch. `items_dev` is a device-resident table (the library reads it on the
 * device); item i owns blocks [first_block, first_block + ntaps * ceil(cout/32) * ceil(cin/32)), first_block ascending
 * from 0; total_blocks = the sum. No tap flip. (backbone_hip.py re-packs all dgrad operands after an optimizer step.) */
typedef struct cms_pack_item {
    const void* src;       /* (ntaps, cout, cin) fp32 or bf16 (all items the same dtype)                             */
    void* dst;             /* (ntaps, cin, cout) bf16                                                                 */
    const float* scale;    /* per output channel (cout) or NULL                                                       */
    int ntaps, cout, cin;
    int first_block;
} cms_pack_item;

int cms_conv_pack_transpose_batch(const cms_pack_item* items_dev, int n_items, int total_blocks, int src_dtype,
                                  void* stream);
/* (round 6) The same for bf16 sources whose cout AND cin are multiples of 64 (every body convolution of the DeepLab networks):
 * 64 x 64 tiles, 16-byte accesses on both sides; item i owns blocks [first_block, first_block + ntaps * (cout/64) * (cin/64)). */
int cms_conv_pack_transpose_batch64(const cms_pack_item* items_dev, int n_items, int total_blocks, void* stream);

/* dW[tap][co][ci] (fp32) += scale[co] * sum over pixels of dU[pix][co] * X[pix shifted by tap][ci]; K = pixels,
 * split across workgroups and accumulated with atomics (zero the gradient buffer once per step). */
typedef struct cms_wgrad_desc {
    const void* du;        /* bf16 [N][ho][wo][cout]: gradient wrt the conv+BN output (pre-activation)            */
    const void* x;         /* bf16 [N][h][w_in][cin]: the conv's input                                             */
    float* dw;             /* fp32 [ntaps][cout][cin]                                                              */
    const float* scale;    /* [cout] frozen-BN scale or NULL                                                       */
    int n, h, w_in, cin, ho, wo, cout;
    int cout_real;         /* rows >= cout_real are skipped (padded class axis); 0 = cout                          */
    int ntaps;
    int tap_dy[CMS_CONV_MAX_TAPS], tap_dx[CMS_CONV_MAX_TAPS];
    int stride;
    int ksplit;            /* 0 = auto                                                                             */
    /* Optional side outputs for a TRAINABLE BatchNorm affine behind the convolution (frozen statistics; torchvision
     * style backbones, architectures/deeplab3plus.py:89-98): with G = the unscaled weight gradient sum_p dU x,
     *   wdot[co]  += <W[.][co][.], G[.][co][.]>  (over taps and input channels; W = the bf16 forward operand)
     *   dbeta[co] += sum over pixels of dU[pix][co]
     * from which  d(bias) = dbeta  and  d(weight) = (wdot - running_mean * dbeta) / sqrt(running_var + eps)  --
     * exact, and no division by the BatchNorm weight. All three NULL = off.                                          */
    const void* w;         /* bf16 [ntaps][cout][cin]                                                              */
    float* wdot;           /* fp32 [cout], accumulated with atomics                                                */
    float* dbeta;          /* fp32 [cout], accumulated with atomics                                                */
    int dw_cout;           /* rows per tap of the dw TENSOR when it is narrower than the GEMM's (padded) cout: the ASPP
                              head computes 64 padded class rows and writes the cout_real live ones straight into the
                              (9, C, 2048) gradient tensor; 0 = cout                                               */
    void* workspace;       /* optional scratch for the split-K partial sums (bf16 entry point), at least
                              cms_conv_wgrad_workspace_bytes(d) long: the pixel slices then write their tiles there with
                              plain stores and a second launch on the same stream adds them to dw IN SLICE ORDER --
                              run-to-run deterministic weight gradients (train_seg_semisup_mask_mt.py:459,465 on the
                              reference's CPU path are deterministic too). NULL or too small: fp32 atomics, whose order
                              varies from run to run (6 % slower alone, 1.5-2 % FASTER inside the two-stream step: the
                              throughput default). The scratch must not be shared by launches that may overlap.       */
    long long workspace_bytes;
    int wg_target;         /* eight-phase kernel only: workgroups (= CUs, one each) this launch should aim at; 0 = the whole
                              machine (a launch that runs alone). A caller that runs weight gradients BESIDE other work says
                              how many CUs are theirs: the DeepLab v2 executor passes 56 per launch on two streams next to
                              the data-gradient chain                                                 */
} cms_wgrad_desc;

int cms_conv_wgrad(const cms_wgrad_desc* d, void* stream);
/* Kernel selection of cms_conv_wgrad (diagnostic / A-B switch; production leaves it alone). Launches with Cout % 256 == 0,
 * Cin % 256 == 0, no BatchNorm-affine side outputs and >= 1024 pixels take the eight-phase 256 x 256 kernel of csrc/wgrad8.hip
 * (few pixel slices, 40-170 K tiles per workgroup), everything else the 128 x 128 kernel of csrc/conv.hip.
 *   mode -1 = the environment decides (CMS_WGRAD8, default 1), 0 = never the eight-phase kernel, 1 = wherever supported. */
int cms_conv_set_wgrad8(int mode);
int cms_conv_wgrad_uses_wgrad8(const cms_wgrad_desc* d);   /* 1: cms_conv_wgrad(d) would take the eight-phase kernel now */

/* GROUPED weight gradients (round 4): the launches of MANY layers -- the bottlenecks of a stretch of the backward pass, autograd
 * of architectures/deeplab2.py:89-109 -- as ONE grid. A per-layer launch has 16 ... 144 output tiles and needs 8 ... 21 pixel
 * slices to occupy the machine; each slice workgroup then runs ~25 pixel stages per 64 KB atomic epilogue. In a group the tiles
 * of all layers fill the machine together (2-3 slices, ~200 stages per epilogue, 3-4 workgroups per CU).
 *   cms_conv_wgrad_group_kind   0 = this launch cannot join a group (channel counts not multiples of 128, side outputs, a
 *                               workspace, padded class axis), 1 = group of pointwise launches, 2 = group of launches with taps
 *   cms_conv_wgrad_group_bytes  size of the item table for n launches
 *   cms_conv_wgrad_group_pack   fills the HOST image of the table for n launches of ONE kind; the caller copies it to the device
 *                               (once per recorded pass) -- target_workgroups: 0 = default; -> grid size in *total_blocks
 *   cms_conv_wgrad_group_run    the launch: table_dev = the device copy                                                        */
int cms_conv_wgrad_group_kind(const cms_wgrad_desc* d);
long long cms_conv_wgrad_group_bytes(int n_items);
int cms_conv_wgrad_group_pack(const cms_wgrad_desc* descs, int n, int target_workgroups, void* host_table, long long bytes,
                              int* total_blocks);
int cms_conv_wgrad_group_run(const void* table_dev, int n_items, int total_blocks, int kind, void* stream);
/* bytes of `workspace` that make the launch deterministic (0: it has a single pixel slice and already is) */
long long cms_conv_wgrad_workspace_bytes(const cms_wgrad_desc* d);

/* ------------------------------------------------------------------------------------------------------------
 * The same convolution family in fp32 on the f32-input MFMA (v_mfma_f32_32x32x2_f32): the PARITY configuration
 * (losses / IoU within 1e-4 of the fp32 reference path) and the precision of the VAT direction
 * pass (train_seg_semisup_vat_mt.py:228-301). Same descriptors; every tensor the bf16 entry points take as bf16 is
 * fp32 here (x, w, y, res, mask_src; du, x of the weight gradient); Cin % 32 == 0; `tile`, `zeros`, `variant` and the
 * BatchNorm-affine side outputs of the weight gradient are not used.
 * ------------------------------------------------------------------------------------------------------------ */
int cms_conv_igemm_f32(const cms_conv_desc* d, void* stream);
int cms_conv_wgrad_f32(const cms_wgrad_desc* d, void* stream);
/* dst[tap'][ci][co] = src[tap][co][ci] * scale[co], fp32 -> fp32 */
int cms_conv_pack_transpose_f32(const float* src, float* dst, const float* scale, int ntaps, int cout, int cin,
                                int flip, void* stream);
/* cms_conv_pack_transpose_batch with fp32 sources AND fp32 destinations */
int cms_conv_pack_transpose_batch_f32(const cms_pack_item* items_dev, int n_items, int total_blocks, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-side input staging (csrc/augment.hip): crop with random scale, flips, ColorJitter / RandomGrayscale,
 * standardisation and NCHW conversion of uint8 source images resident in HBM -- the loader-worker transforms of
 * datapipe/seg_transforms_cv.py:29-133, 169-231, 452-497, 541-623 as wired at train_seg_semisup_mask_mt.py:150-183.
 * params[n][CMS_AUG_PARAMS] (DEVICE, float), drawn on the host in the reference's order:
 *   0 y0, 1 x0   window origin in (unpadded) source pixels, may be negative (padding: image 0 after standardisation,
 *                label 255, mask 0)         2 sc_h, 3 sc_w   window size (== h, w without random scale)
 *   4 flip_x, 5 flip_y, 6 transpose (0/1)   7 brightness, 8 contrast, 9 saturation factors, 10 hue shift (turns)
 *   11 greyscale (0/1)   12 colour jitter applied (0/1)   13 order of the four jitter ops, base-4 digits
 *   14 contrast pivot (mean luminance; fill with cms_augment_luma x brightness when brightness comes first)
 *   15 geometry: 0 = the axis-aligned window of slots 0..3 (crop / Hung scale, above); 1 = AFFINE WARP, the random
 *      rotate + scale crop of datapipe/seg_transforms_cv.py:306-372 (cv2.warpAffine): output pixel (x, y) samples the
 *      source at (a00 x + a01 y + a02, a10 x + a11 y + a12) with slots 16..21 = a00 a01 a02 a10 a11 a12 (the INVERSE of
 *      the reference's local_xf), slot 22 = interpolation of the image (0 nearest: floor(s + 0.5); 1 bilinear), image
 *      border REFLECT_101, labels nearest with 255 outside, mask = in-bounds weight (constant border 0)
 *   23 mask mode (either geometry): 0 = the mask is the in-bounds weight of the image taps (cv2.INTER_LINEAR of the mask, what a
 *      single view gets); 1 = the mask is 1 exactly when the NEAREST source pixel -- the one the labels are read from -- lies
 *      inside the source, else 0 (cv2.INTER_NEAREST of the mask: view 1 of a Hung scale-crop PAIR, seg_transforms_cv.py:272).
 *      The image and its zero padding do not depend on it.
 * out0 = geometric transform only (teacher view), out1 = + colour augmentation (student view); either may be NULL.
 * ------------------------------------------------------------------------------------------------------------ */
#define CMS_AUG_PARAMS 24
typedef struct cms_augment_desc {
    const uint8_t* src;         /* uint8 [N][hs][ws][3]                                  */
    const uint8_t* src_labels;  /* uint8 [N][hs][ws] or NULL                             */
    void* out0;                 /* (N,3,h,w) NCHW, out_dtype, or NULL                    */
    void* out1;                 /* (N,3,h,w) NCHW, out_dtype, or NULL                    */
    uint8_t* out_labels;        /* (N,h,w) uint8 or NULL (255 outside the source image)  */
    float* out_mask;            /* (N,1,h,w) fp32 validity mask or NULL                  */
    const float* params;        /* DEVICE [N][CMS_AUG_PARAMS]                            */
    float mean[3], std_[3];     /* standardisation (seg_transforms_cv.py:600-612)        */
    int n, hs, ws, h, w;
    int out_dtype;
} cms_augment_desc;
int cms_augment_batch(const cms_augment_desc* d, void* stream);
/* luma[n] = mean luminance in [0,1] of sample n after its geometric transform (ColorJitter's contrast pivot) */
int cms_augment_luma(const cms_augment_desc* d, float* luma, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Ragged staging (csrc/stage.hip): the same transform, every batch sample gathered from its own entry of a pool of
 * VARIABLE-SIZED uint8 images resident in HBM (data sets whose images differ in size: Pascal VOC). Entry e of the pool is
 * [hs][ws][3] uint8 at pool_img + entries[e].img_off and, with labels, [hs][ws] uint8 at pool_labels + entries[e].lab_off
 * (dense rows; 64-bit byte offsets: pools exceed 4 GB). index[n] names the entry of batch sample n (any order, repeats
 * allowed). params / outputs / mean / std_ / out_dtype: exactly cms_augment_desc's, slot meanings unchanged; with entries of
 * one size and index = 0..n-1 the outputs are cms_augment_batch's bit for bit. Nothing outside an entry's hs * ws pixels is
 * read: window taps are bounds-tested, warp taps reflected; an index outside [0, n_entries) or an entry with a non-positive
 * size stages as an empty source (image 0, labels 255, mask 0). Whole-image evaluation staging (datapipe/seg_data.py:181-216,
 * 246-273: standardise, centre on a canvas padded with image 0 / label 255) is window mode with origin (-dh // 2, -dw // 2),
 * window = canvas = (h, w).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct cms_stage_entry {
    long long img_off;          /* byte offset of the entry's pixels in pool_img (16-byte aligned)   */
    long long lab_off;          /* byte offset of its label map in pool_labels, or -1                */
    int hs, ws;                 /* its size                                                          */
} cms_stage_entry;
typedef struct cms_stage_desc {
    const uint8_t* pool_img;    /* uint8 pool of images                                  */
    const uint8_t* pool_labels; /* uint8 pool of label maps or NULL                      */
    const cms_stage_entry* entries; /* DEVICE [n_entries]                                */
    const int* index;           /* DEVICE int32 [n]: pool entry of each batch sample     */
    void* out0;                 /* (N,3,h,w) NCHW, out_dtype, or NULL                    */
    void* out1;                 /* (N,3,h,w) NCHW, out_dtype, or NULL                    */
    uint8_t* out_labels;        /* (N,h,w) uint8 or NULL (255 outside the source image)  */
    float* out_mask;            /* (N,1,h,w) fp32 validity mask or NULL                  */
    const float* params;        /* DEVICE [N][CMS_AUG_PARAMS]                            */
    float mean[3], std_[3];
    int n, n_entries, h, w;
    int out_dtype;
} cms_stage_desc;
int cms_stage_batch(const cms_stage_desc* d, void* stream);
/* luma[n] as cms_augment_luma, for the ragged source */
int cms_stage_luma(const cms_stage_desc* d, float* luma, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Batch-statistics BatchNorm (+ ReLU, + residual) on NHWC activations (csrc/bn.hip): nn.BatchNorm2d in training mode,
 * architectures/deeplab2.py:72-84 without --freeze_bn, architectures/deeplab3plus.py:40-64 (head, always).
 * ONE descriptor (cms_bn_op) and ONE launch entry point (cms_bn_run, or cms_program_add_bn inside a recorded program);
 * `what` names the launch, the fields a kind does not list are ignored (leave them NULL / 0):
 *   forward : REDUCE -> sums = (sum x, sum x^2);  FINALIZE -> mean, rstd, scale, shift and the running statistics (momentum,
 *             unbiased variance);  APPLY: y = relu(x*scale + shift (+ res)).
 *             STATS = REDUCE + FINALIZE in one launch (single-process callers); FINALIZE_TILES = the same from the tile sums
 *             the unit's convolution wrote (cms_conv_desc.stats_out): no pass over x at all.
 *   backward: REDUCE_BWD -> sums = (sum dy', sum dy'*xhat), dy' = dy * [y > 0] (no mask given: no ReLU); BWD_SUMS_TILES = the
 *             same from the tile sums of the data-gradient launch that wrote dy (cms_conv_desc.bstats_*);
 *             BWD_APPLY: dx = gamma*rstd*(dy' - sums0/count - xhat*sums1/count), optional dres = dy'.
 *             dgamma = sums1, dbeta = sums0 (of the LOCAL pass).
 *   COUNT   : *counter += 1 (cms_increment_counter as a program op).
 * Statistics are a two-pass protocol so that a data-parallel caller can all-reduce `sums` between the passes (SyncBN,
 * SURVEY.md 8(e)): forward between REDUCE and FINALIZE, backward between REDUCE_BWD / BWD_SUMS_TILES and BWD_APPLY, with
 * `count` = the pixels of one group on ALL ranks. STATS and FINALIZE_TILES take count = n_pixels / groups themselves.
 * Sample groups (`groups` >= 1, dividing n_pixels): the pixel rows are `groups` equal runs of consecutive samples whose
 * statistics are kept apart -- ONE launch over [supervised batch; mixed batch] normalises each exactly as the reference's
 * separate forward passes do (train_seg_semisup_mask_mt.py:296-358); the running statistics move once per group, in group
 * order, `counter` by `groups`. Layouts with groups: mean / rstd / scale / shift float[groups][c], sums double[groups][2][c].
 * FINALIZE handles ONE group of c channels (a grouped caller issues it per group on slices of sums / mean / ... ).
 * ------------------------------------------------------------------------------------------------------------ */
enum cms_bn_what { CMS_BN_REDUCE = 0, CMS_BN_FINALIZE, CMS_BN_APPLY, CMS_BN_REDUCE_BWD, CMS_BN_BWD_APPLY, CMS_BN_COUNT,
                   CMS_BN_STATS, CMS_BN_FINALIZE_TILES, CMS_BN_BWD_SUMS_TILES };

typedef struct cms_bn_op {
    int what;                  /* enum cms_bn_what                                                             */
    int dtype, c, relu;        /* of x / y / dy / dx / dres; channels (c % 8 == 0); APPLY: ReLU                */
    const void* x;             /* conv output u, NHWC                                                          */
    const void* res;           /* APPLY: residual or NULL                                                      */
    void* y;                   /* APPLY: output; REDUCE_BWD / BWD_APPLY: the stored output (ReLU mask) or NULL */
    const void* dy;            /* backward: incoming gradient                                                  */
    void* dx;                  /* BWD_APPLY: gradient wrt x                                                    */
    void* dres;                /* BWD_APPLY: gradient wrt the residual (= masked dy) or NULL                   */
    double* sums;              /* double[groups][2][c]. Without `ws`, REDUCE / REDUCE_BWD ACCUMULATE into it with atomics (the
                                * caller zero-fills; layers wider than 2048 channels run as channel slices); with `ws` and from
                                * BWD_SUMS_TILES it is OVERWRITTEN, bit-reproducibly. STATS: optional copy of the sums (NULL: not
                                * written). Read by FINALIZE and BWD_APPLY                                                     */
    const float* gamma;        /* FINALIZE / STATS / FINALIZE_TILES / BWD_APPLY; NULL = 1                      */
    const float* beta;         /* NULL = 0                                                                     */
    float* mean;               /* written by FINALIZE / STATS / FINALIZE_TILES, read by the backward kinds     */
    float* rstd;
    float* scale;              /* gamma * rstd: written like mean, read by APPLY                               */
    float* shift;              /* beta - mean * scale                                                          */
    float* running_mean;       /* FINALIZE / STATS / FINALIZE_TILES: moved like nn.BatchNorm2d's, or NULL      */
    float* running_var;
    long long* counter;        /* num_batches_tracked: COUNT; optional for FINALIZE (+ 1) and STATS / FINALIZE_TILES (+ groups) */
    double* clear_a;           /* FINALIZE: double[2*c] each, zeroed after the statistics were read -- normally the forward sums   */
    double* clear_b;           /* themselves and the sums of the unit's backward pass, for their next replay -- or NULL            */
    void* ws;                  /* REDUCE / REDUCE_BWD (optional; needed for groups > 1 and for mask_bits) and STATS: the reductions
                                * WITHOUT data atomics -- blocks own 64-channel tiles, store partial sums here and the last block of a
                                * tile adds them in fixed order in fp64. cms_bn_workspace_bytes(n_pixels, c, groups) bytes, zero-filled
                                * once by the caller, owned by one call site (launches on different streams must not share it), left
                                * ready for the next launch. FINALIZE_TILES / BWD_SUMS_TILES: the tile sums instead, float
                                * [tiles][2 slots][2][c] as cms_conv_desc.stats_out describes them                                 */
    double count;              /* FINALIZE / BWD_APPLY: pixels the statistics of ONE group run over            */
    unsigned long long n_pixels; /* pixel rows of x (all groups)                                               */
    float eps, momentum;
    int groups;                /* sample groups (0 / 1: one)                                                   */
    int tile_rows;             /* FINALIZE_TILES / BWD_SUMS_TILES: pixel rows per statistics tile (cms_conv_igemm_stats_tile_rows of
                                * the launch that wrote them); a group is at least one tile long, groups <= 64 */
    void* mask_bits;           /* the ReLU mask as BITS beside y -- uint8 [pixel rows][c / 8], bit e of byte (row, v) = [stored
                                * y[row][8 v + e] > 0], the layout of cms_conv_desc.mask_bits_out. APPLY writes them (or NULL);
                                * REDUCE_BWD (with ws) and BWD_APPLY read them INSTEAD of y: 1/16 of the bytes of one of the three
                                * tensors they stream, bit-identical results. NULL: y is the mask                                  */
} cms_bn_op;

size_t cms_bn_workspace_bytes(size_t n_pixels, int c, int groups);
int cms_bn_run(const cms_bn_op* op, void* stream);
/* Backward of y = relu(x * scale + shift (+ res)) with FROZEN statistics (an eval-mode BatchNorm as an affine: the forward is
 * CMS_BN_APPLY with scale = gamma * rstd, shift = beta - mean * scale; architectures/deeplab2.py LayerEngine.bn_act, the teacher of
 * train_seg_semisup_vat_mt.py:237): dx = scale * dy', dres = dy' (or NULL), dy' = dy * [y > 0] (y = the forward's output; NULL: no ReLU). */
int cms_frozen_bn_act_bwd(const void* dy, const void* y, void* dx, void* dres, int dtype, const float* scale, size_t n_pixels, int c,
                          void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * NHWC data movement of the DeepLab v3+ head (csrc/nhwc.hip; reference: architectures/deeplab3plus.py:40-55 -- torch.cat of
 * the ASPP branches, the pooled branch broadcast over the map, F.interpolate(bilinear, align_corners=False) + torch.cat with
 * the low-level features -- and autograd's sum of the gradients that meet at the ASPP input). Pixel rows may sit in wider
 * rows of a concat buffer: `*_pitch` = elements per row of that buffer; rows, pitches and pointers are multiples of 16 bytes.
 *   cms_channel_copy : dst[r][0:channels] = src[r / row_div][0:channels]   (row_div > 1 broadcasts one row per sample)
 *   cms_add_n        : dst = src_0 + ... + src_{k-1}, k <= 6, fp32 accumulation, dense tensors of n elements (n % 8 == 0)
 *   cms_rows_reduce  : dst[n][c] (fp32) = scale * sum_p src[n][p][c]        (global average pool; adjoint of the broadcast)
 *   cms_upsample_nhwc: backward == 0: dst[N,H,W, pitch] <- bilinear(src[N,h,w,C]); backward != 0: the adjoint in gather form,
 *                      src = d(dst) in rows of dst_pitch, dst = d(src) dense (N,h,w,C). No atomics, fixed summation order.
 * ------------------------------------------------------------------------------------------------------------ */
int cms_channel_copy(const void* src, size_t src_pitch, void* dst, size_t dst_pitch, size_t rows, int channels, int dtype,
                     size_t row_div, void* stream);
int cms_add_n(const void* const* srcs, int k, void* dst, size_t n, int dtype, void* stream);
int cms_rows_reduce(const void* src, size_t pitch, int n, size_t rows_per_sample, int channels, int dtype, float* dst,
                    float scale, void* stream);
int cms_upsample_nhwc(const void* src, void* dst, size_t dst_pitch, int n, int h, int w, int H, int W, int channels, int dtype,
                      int align_corners, int backward, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * ASPP head (architectures/deeplab2.py:112-128) with the 2048-channel activation read ONCE (csrc/aspp.hip):
 *   forward   Z = X . Wall^T as a 1x1 cms_conv_igemm (rows of Wall: tap*C + class, fp32 NCHW output), then
 *             logits[n][c][y][x] = bias[c] + sum_t Z[n][t*C + c][y + dy_t][x + dx_t]            (cms_aspp_gather_fwd)
 *   backward  D[n][y][x][t*C + c] = dlogits[n][c][y - dy_t][x - dx_t]                             (cms_aspp_spread_bwd),
 *             then dX = D . Wall (1x1 cms_conv_igemm) and dWall = D^T . X (one cms_conv_wgrad).
 * zc = channel count of Z / D (taps * classes padded to what the GEMMs need); columns >= taps * classes are zero.
 * ------------------------------------------------------------------------------------------------------------ */
int cms_aspp_gather_fwd(const float* z, const float* bias, float* logits, const int* tap_dy, const int* tap_dx, int n_taps,
                        int n, int c, int zc, int h, int w, void* stream);
int cms_aspp_spread_bwd(const float* dlogits, void* d_nhwc, int d_dtype, const int* tap_dy, const int* tap_dx, int n_taps,
                        int n, int c, int zc, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Network stem: 7x7 / stride 2 / pad 3 convolution 3 -> 64 + frozen BatchNorm + ReLU, 3x3 / stride 2 / pad 1 ceil-mode
 * max-pool, and their backward passes (architectures/deeplab2.py:140-146, 183-186; csrc/stem.hip).
 * Images NCHW (the reference's batch layout), activations NHWC; dtypes CMS_F32 / CMS_BF16 per tensor.
 * ------------------------------------------------------------------------------------------------------------ */
/* w_packed[(c*7 + ky)*7 + kx][co] (fp32, 147 x 64) from the convolution weight in its [kh][kw][Cout][Cin] layout,
 * followed by the bf16 (hi, lo) MFMA fragments of the bf16 forward: the buffer holds (147 + 176) x 64 floats. */
int cms_stem_pack_weights(const void* w_khkwcoci, int w_dtype, float* w_packed, void* stream);
/* sizes of the stem convolution output (ho, wo) and of the max-pool output (hp, wp) for an h x w image */
int cms_stem_out_hw(int h, int w, int* ho, int* wo, int* hp, int* wp);
/* y[n][oy][ox][co] = relu(conv(x)[co] * scale[co] + bias[co]) */
int cms_stem_fwd(const void* x_nchw, int x_dtype, void* y_nhwc, int y_dtype, const float* w_packed, const float* scale,
                 const float* bias, int n, int h, int w, void* stream);
/* ceil_mode 1: DeepLab v2 (deeplab2.py:146); 0: torchvision's ResNet stem (DeepLab v3+ backbone).
 * p = maxpool(s); argmax[n][py][px][c] = ky*3+kx of the FIRST maximum of the window (ATen's rule) */
int cms_maxpool3x3s2_fwd(const void* s_nhwc, void* p_nhwc, uint8_t* argmax, int dtype, int n, int hs, int ws, int c,
                         int ceil_mode, void* stream);
/* ds = [s > 0] * scatter(dp through argmax): max-pool backward fused with the ReLU backward of its input */
int cms_maxpool3x3s2_relu_bwd(const void* dp_nhwc, const uint8_t* argmax, const void* s_nhwc, void* ds_nhwc, int dtype,
                              int n, int hs, int ws, int c, int ceil_mode, void* stream);
/* dw[ky][kx][co][c] (fp32, accumulated with atomics) += scale[co] * sum_pixels ds[pix][co] * x[c][2oy-3+ky][2ox-3+kx] */
int cms_stem_wgrad(const void* x_nchw, int x_dtype, const void* ds_nhwc, int ds_dtype, float* dw_khkwcoci,
                   const float* scale, int n, int h, int w, void* stream);
/* The same with an optional scratch buffer (>= cms_stem_wgrad_workspace_bytes): the persistent blocks then write their
 * partial sums there and a second launch adds them to dw in block order -- run-to-run DETERMINISTIC (NULL: fp32 atomics). */
long long cms_stem_wgrad_workspace_bytes(int x_dtype, int ds_dtype, int n, int h, int w);
int cms_stem_wgrad_ws(const void* x_nchw, int x_dtype, const void* ds_nhwc, int ds_dtype, float* dw_khkwcoci,
                      const float* scale, int n, int h, int w, void* workspace, long long workspace_bytes, void* stream);
/* dx (fp32 NCHW) = gradient wrt the image (VAT direction pass, train_seg_semisup_vat_mt.py:244-268) */
int cms_stem_dgrad(const void* ds_nhwc, int ds_dtype, const float* w_packed, const float* scale, float* dx_nchw, int n,
                   int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Launch programs: the host side of a network pass, recorded once per input shape and replayed from C++
 * (csrc/program.hip). Replaces one Python -> ctypes round trip per convolution of architectures/deeplab2.py:89-128
 * (and of its backward pass) by ONE call per pass. Ops refer to caller-owned, persistent device buffers; stream
 * indices are positions in the `streams` array given at run time (index 0 = the caller's current stream).
 * add_* return the op index (>= 0) or a negative error code.
 * ------------------------------------------------------------------------------------------------------------ */
#define CMS_PROGRAM_MAX_STREAMS 4
typedef struct cms_program cms_program;
int cms_program_create(cms_program** out);
int cms_program_destroy(cms_program* p);
int cms_program_add_conv(cms_program* p, const cms_conv_desc* d, int f32, int stream_idx, int group);
int cms_program_add_wgrad(cms_program* p, const cms_wgrad_desc* d, int f32, int stream_idx, int group);
/* a grouped weight-gradient launch (cms_conv_wgrad_group_run) as a program op */
int cms_program_add_wgrad_group(cms_program* p, const void* table_dev, int n_items, int total_blocks, int kind, int stream_idx,
                                int group);
int cms_program_add_memset(cms_program* p, void* ptr, size_t bytes, int stream_idx, int group);
int cms_program_add_aspp_gather(cms_program* p, const float* z, const float* bias, float* logits, const int* tap_dy,
                                const int* tap_dx, int n_taps, int n, int c, int zc, int h, int w, int stream_idx, int group);
int cms_program_add_aspp_spread(cms_program* p, const float* dlogits, void* d_nhwc, int d_dtype, const int* tap_dy,
                                const int* tap_dx, int n_taps, int n, int c, int zc, int h, int w, int stream_idx, int group);
/* work enqueued so far on `from_stream` must finish before anything enqueued later on `to_stream` starts */
int cms_program_add_sync(cms_program* p, int from_stream, int to_stream, int group);
/* Trainable BatchNorm affine over frozen statistics on the eight-phase weight-gradient kernel (csrc/wfinish.hip; the torchvision
 * backbone of architectures/deeplab3plus.py:96-98 + autograd): the weight-gradient launch writes the UNSCALED gradient G into a
 * scratch tensor of the weight's shape, cms_channel_sum takes d(beta) = sum_p dU, and one finishing launch per backward pass does,
 * per item and output channel co:  grad += scale[co] * G,  wdot[co] += <W[co], G[co]>,  G = 0.  All buffers are the caller's. */
typedef struct cms_wfinish_item {
    float* scratch;            /* fp32 [ntaps][cout][cin]: G of this pass, cleared by the launch                         */
    float* grad;               /* fp32 [ntaps][cout][cin]: the gradient arena's slice of the weight                      */
    const uint16_t* w;         /* bf16 [ntaps][cout][cin]: the weight                                                    */
    const float* scale;        /* [cout] gamma * rstd, or NULL (1)                                                        */
    float* wdot;               /* [cout], accumulated                                                                     */
    int ntaps, cout, cin;      /* cin % 4 == 0                                                                            */
    int first_block;           /* filled by cms_wgrad_finish_pack                                                         */
} cms_wfinish_item;
/* dst[c] (fp32, accumulated with atomics) += sum over `rows` rows of src[row][c]; channels % 64 == 0 */
int cms_channel_sum(const void* src, int dtype, size_t rows, int channels, float* dst, void* stream);
/* host: lays the items out over the grid (first_block) -> total workgroups, or a negative error code */
int cms_wgrad_finish_pack(cms_wfinish_item* items, int n_items);
/* items_dev: the packed table in device memory */
int cms_wgrad_finish_run(const void* items_dev, int n_items, int total_blocks, void* stream);
/* ... as program ops */
int cms_program_add_channel_sum(cms_program* p, const void* src, int dtype, size_t rows, int channels, float* dst, int stream_idx,
                                int group);
int cms_program_add_wgrad_finish(cms_program* p, const void* items_dev, int n_items, int total_blocks, int stream_idx, int group);

/* A cms_bn_run launch inside a program (DeepLab v2 WITHOUT --freeze_bn on the executor, architectures/deeplab2.py:72-84 /
 * train_seg_semisup_mask_mt.py:587). All buffers are the caller's and persistent (a program is replayed many times). */
int cms_program_add_bn(cms_program* p, const cms_bn_op* op, int stream_idx, int group);
int cms_program_size(const cms_program* p);
/* enqueue ops [first, last) (last < 0: to the end); never synchronises the host */
int cms_program_run(cms_program* p, int first, int last, void* const* streams, int n_streams);
/* two programs issued interleaved by `group` (student on one stream, teacher on another) */
int cms_program_run_pair(cms_program* a, void* const* streams_a, int na, cms_program* b, void* const* streams_b, int nb);
/* bracket every k-th convolution launch with HIP events on its stream (0 = off) / read and reset the sums */
int cms_program_set_timing(cms_program* p, int every_k);
/* the ASPP head launches (fp32 NCHW output) are always bracketed while timing is on and summed separately */
int cms_program_read_timing(cms_program* p, double* sum_ms, double* sum_flops, long* launches, double* head_ms,
                            long* head_launches);

/* ------------------------------------------------------------------------------------------------------------
 * Batched 2-D complex fp64 FFT (csrc/fft.hip), the transform under the patch-distance analysis below.
 *   data   (batch, fh, fw) interleaved complex128, transformed IN PLACE; fh, fw powers of two in 8 ... 4096, batch <= 65535
 *   tw_h, tw_w   DEVICE tables of fh / 2 and fw / 2 complex128: exp(-2 pi i k / n), built by the caller in float64 (the same
 *          table serves both directions; one table may be passed twice when fh == fw)
 *   inverse != 0: the inverse transform, scaled by 1 / (fh * fw)
 * Two stream-ordered launches (rows, then tiles of adjacent columns), both with their data in LDS.
 * ------------------------------------------------------------------------------------------------------------ */
int cms_fft2(void* data, int batch, int fh, int fw, int inverse, const void* tw_h, const void* tw_w, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Patch distances (csrc/patchdist.hip): patch_dist.py:107-154 sliding_window_distance_to_patch[es_generator] and
 * intra_inter_class_patch_dist.py:186-211, on exact integer grey levels. For a (ph, pw, 3) patch Q[n] and an image symmetric-padded
 * by ((ph - 1) / 2, (pw - 1) / 2) (numpy's `symmetric`: the edge pixel repeats, any number of reflections):
 *     D2[n,i,j] = P2[i,j] + Q2[n] - 2 PQ[n,i,j]       PQ = the `valid` cross-correlation, from the fp64 FFT, rounded to integers
 * ph, pw odd; FFT sizes fh >= hs + ph - 1, fw >= ws + pw - 1 as cms_fft2 takes them. The call sequence per image and chunk of n
 * patches: load_image, load_patches, cms_fft2 on both, spectrum_product, cms_fft2 inverse, finish, select_k_smallest.
 *   cms_pd_load_image      pool entry (uint8 [hs][ws][3] at pool_img + entry_host->img_off; entry_host is a HOST pointer) ->
 *                          planes (3, fh, fw) complex128: the padded image, imaginary part and everything past it zero;
 *                          sq (hs + ph - 1, ws + pw - 1) int64 = sum over channels of the padded image squared, or NULL
 *   cms_pd_load_patches    patches[n] = where patch n is cut: the pool entry and the centre (cy, cx) in it (cut from the padded
 *                          entry, so any centre inside the entry is valid) -> planes ((n + 1) / 2, 3, fh, fw) complex128: pair k
 *                          holds patch 2k FLIPPED in the real part and patch 2k + 1 flipped in the imaginary part (zero when
 *                          n is odd and 2k + 1 == n), so that F_image * F_pair needs no conjugate
 *   cms_pd_patch_sqdiff    out[n] = sum over the patch of (a[n] - b[n])^2, or of a[n]^2 when b is NULL (that is Q2), int64
 *   cms_pd_spectrum_product out (n_pairs, fh, fw) = sum over the 3 channels of f_img[c] * f_pairs[k][c]
 *   cms_pd_finish          corr = the inverse transform of that product; p2 (h, w) int64 box sums of sq; q2 (n) ->
 *                          d2 (n, h, w) int64 and / or keys (n, h * w) int64 = D2 << 24 | flat index (h * w <= 2^24);
 *                          *residual_bits = max(*residual_bits, bit pattern of the largest |re - rint(re)| of the launch): the
 *                          caller zeroes it, and refuses the result when the value is not far below 0.5 (NaN if not finite)
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct cms_pd_patch {
    long long img_off;          /* byte offset of the patch's pool entry in pool_img                */
    int hs, ws;                 /* size of that entry                                               */
    int cy, cx;                 /* centre of the patch in it                                        */
} cms_pd_patch;
int cms_pd_load_image(const uint8_t* pool_img, const cms_stage_entry* entry_host, int ph, int pw, int fh, int fw, void* planes,
                      int64_t* sq, void* stream);
int cms_pd_load_patches(const uint8_t* pool_img, const cms_pd_patch* patches, int n, int ph, int pw, int fh, int fw, void* planes,
                        void* stream);
int cms_pd_patch_sqdiff(const uint8_t* pool_img, const cms_pd_patch* a, const cms_pd_patch* b, int n, int ph, int pw, int64_t* out,
                        void* stream);
int cms_pd_spectrum_product(const void* f_img, const void* f_pairs, int n_pairs, int fh, int fw, void* out, void* stream);
int cms_pd_finish(const void* corr, const int64_t* p2, const int64_t* q2, int n, int h, int w, int fh, int fw, int64_t* d2,
                  int64_t* keys, uint64_t* residual_bits, void* stream);
/* The k smallest masked keys of each of n rows of m non-negative int64 keys (radix select: eight 8-bit histogram passes find the
 * k-th key, one pass compacts the keys <= it; no sort). The candidates of row r are, by `mode`:
 *     0  mask[r][i] != 0 (mask (n, m) uint8)      1  labels[i] == cls[r]      2  labels[i] != cls[r] and labels[i] != 255
 * (labels (m) uint8 shared by every row, cls (n) int32). out (n, k) int64: the selected keys of a row in NO particular order, the
 * rest of the row INT64_MAX; count[r] = how many (min(k, candidates) when the keys of a row are distinct). workspace:
 * cms_select_workspace_bytes(n) bytes. */
size_t cms_select_workspace_bytes(int n);
int cms_select_k_smallest(const int64_t* keys, const uint8_t* mask, const uint8_t* labels, const int32_t* cls, int mode, int n,
                          long long m, int k, int64_t* out, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* Neighbouring-patch distances (patch_dist.py:39-104 box_sum, neighbouring_patch_distance_maps): for every pixel of a pool entry the
 * squared distance, in integer grey levels, between the (ph, pw, 3) patch centred on it and the patches centred on its left, right,
 * upper and lower neighbour, all cut from the entry symmetric-padded by ((ph - 1) / 2 + 1, (pw - 1) / 2 + 1). Shifting a patch by
 * one pixel makes that a ph x pw box sum of squared neighbour differences; integer arithmetic throughout, no atomics: the results
 * are exact and the same on every run. The reference's distance is sqrt(D2) / 255.
 *   cms_pd_box_sum   in: a plane (hp, wp) of int32 (in_is_int64 == 0) or int64 -> out (hp - ph + 1, wp - pw + 1) int64, the sum of
 *                    every ph x pw window (any ph <= hp, pw <= wp, even ones too; hp * wp < 2^30); sums wrap at 64 bits. Two
 *                    separable running-sum passes: the loads per output do not grow with the box. work: (hp - ph + 1) * wp int64,
 *                    need not be initialised
 *   cms_pd_neighbour_workspace_bytes   bytes of `work` below; 0 for sizes cms_pd_neighbour_maps refuses
 *   cms_pd_neighbour_maps   entry_host as for cms_pd_load_image; ph, pw odd -> out_d2 int64 [4][hs][ws] in the order left, right,
 *                    up, down (< 2^39 for the patch sizes patch_dist accepts). work need not be initialised. Five stream-ordered
 *                    launches: the squared differences (two int32 planes), then two passes per plane pair
 * Bad sizes or NULL pointers return CMS_EINVAL and launch nothing. */
int cms_pd_box_sum(const void* in, int in_is_int64, int hp, int wp, int ph, int pw, void* work, int64_t* out, void* stream);
size_t cms_pd_neighbour_workspace_bytes(int hs, int ws, int ph, int pw);
int cms_pd_neighbour_maps(const uint8_t* pool_img, const cms_stage_entry* entry_host, int ph, int pw, void* work, int64_t* out_d2,
                          void* stream);

/* Downsampling of the Cityscapes converter (convert_cityscapes.py:17-24, 44-46), uint8 in and out, dense tensors:
 *   cms_downsample_image_u8    (n, h, w, 3) -> (n, h / d, w / d, 3): the mean of each d x d block per channel, truncated, which is
 *                    exactly floor(sum / d^2)
 *   cms_downsample_labels_u8   (n, h, w) -> (n, h / d, w / d): the most frequent value of each d x d block, the lowest value among
 *                    equally frequent ones (the reference's one-hot sum and argmax); any byte value is a label
 * d = 1 copies. Integer arithmetic, no atomics: the results are the same on every run. NULL pointers, n < 1, d outside 1..8,
 * h or w not divisible by d, or more than 2^31 - 1 bytes per tensor return CMS_EINVAL, decided before any HIP call; nothing is
 * launched. src and dst must not overlap. */
int cms_downsample_image_u8(const uint8_t* src, int n, int h, int w, int d, uint8_t* dst, void* stream);
int cms_downsample_labels_u8(const uint8_t* src, int n, int h, int w, int d, uint8_t* dst, void* stream);

/* Area resize and statistics of the ISIC 2017 converter (csrc/resize.hip), dense tensors:
 *   cms_resize_area_u8   (n, h, w, c) uint8 -> (n, ho, wo, c), c = 1 or 3, 1 <= ho <= h <= 16384, 1 <= wo <= w <= 16384. Along an
 *                    axis of L pixels and Lo cells, in units of 1 / Lo pixel, pixel i covers [i Lo, (i + 1) Lo), cell o covers
 *                    [o L, (o + 1) L) and wt(o, i) is the length of their overlap; out = sum wy wx p / (h w), rounded to nearest,
 *                    an exact half to the even neighbour. ho == h and wo == w copies. This is the project's own definition of the
 *                    area filter, not cv2's float32 one: see DESIGN section 8
 *   cms_sum_sumsq_u8     (n, pixels, c) uint8, c = 1 or 3 -> sums (n, 2c) int64: the sum of p per channel, then the sum of p^2
 * Integer arithmetic, no atomics: the results are the same on every run. NULL pointers, c other than 1 or 3, a size < 1, ho > h,
 * wo > w, a side above 16384 or more than 2^31 - 1 bytes per tensor return CMS_EINVAL, decided before any HIP call; nothing is
 * launched. src and dst must not overlap. */
int cms_resize_area_u8(const uint8_t* src, int n, int h, int w, int c, int ho, int wo, uint8_t* dst, void* stream);
int cms_sum_sumsq_u8(const uint8_t* src, int n, int pixels, int c, int64_t* sums, void* stream);

/* CowMask (csrc/cowmask.hip): Gaussian-smoothed noise thresholded so that a chosen share of the pixels is 1.
 *   noise          (n, h, w) f32
 *   taps           (n, 2 * radius + 1) double: one row of 1-D weights per sample, applied along x and along y with ZERO padding
 *   thresh_factor  (n) double: tau = mean(s) + std(s) * thresh_factor, the statistics over the sample's smoothed plane s, ddof = 0
 *   mask_out       (n, h, w) f32 = [s <= tau]
 *   stats_out      optional (n, 2) double = { mean, std }
 *   workspace      cms_cowmask_workspace_bytes(n, h, w) bytes of device memory, need not be initialised; that function returns 0
 *                  for sizes cms_cowmask refuses
 * Everything after the f32 noise is fp64. Three stream-ordered launches, no atomics, every sum in a fixed order: the same input
 * gives the same bits, and a sample's mask does not depend on the rest of its batch. NULL pointers (stats_out excepted),
 * n, h or w < 1, radius < 0 or > 128, more than 2^31 - 1 pixels or a workspace that is too small return CMS_EINVAL, decided before
 * any HIP call; nothing is launched. */
size_t cms_cowmask_workspace_bytes(int n, int h, int w);
int cms_cowmask(const float* noise, const double* taps, const double* thresh_factor, int n, int h, int w, int radius,
                float* mask_out, double* stats_out, void* workspace, size_t workspace_bytes, void* stream);

/* Test-time augmentation (csrc/tta.hip): the inputs of the scaled / mirrored views of an evaluation batch, and the vote that fuses
 * the views' low-resolution logits into one prediction. The reference evaluates at one scale without a flip; this goes beyond it.
 *
 * cms_tta_resize: one view's input.
 *   src            (n, c, H, W), dst (n, c, Hs, Ws), both of `dtype` (CMS_F32 / CMS_BF16), dense; must not overlap
 *   dst[.., y, xd] the bilinear sample of src at output pixel (y, x) under align_corners=False (no antialiasing; up- and
 *                  down-scaling alike), xd = flip ? Ws - 1 - x : x. The sample position (y + 0.5) * H / Hs - 0.5 is worked out exactly
 *                  in integers; the interpolation is fp32 in the order of the upsampling kernels, rounded once to `dtype`. Every
 *                  element of dst is written.
 * NULL pointers, a size below 1, an unknown dtype or more than 2^31 - 1 elements in src or dst return CMS_EINVAL.
 *
 * cms_tta_vote: per output pixel (y, x) of (n, H, W), with v_ic the bilinear sample (under `align_corners`) of view i's logits of
 * class c, a flipped view read mirrored along x:
 *   k == 1   score_c = v_0c: prediction, histogram and the identity-size fast path are bit for bit cms_argmax_confusion's, NaN rule
 *            included
 *   k >= 2   score_c = p_0c + p_1c + ..., p_i = softmax(v_i) (max, exponentials summed in class order, one reciprocal, rounded
 *            products), summed in view order in fp32; non-finite logits are outside the contract
 *   pred     the first index of the largest score
 *   logits[i]      (n, c, h[i], w[i]) f32, i < k <= CMS_TTA_MAX_VIEWS; flip[i] != 0: the view was computed on the mirrored input
 *   labels         optional (n, H, W) uint8 / int64 (label_dtype); needed with cm
 *   cm             optional int64 (c, c) += histogram of (label, pred) over pixels with label != ignore_index (< 0: none)
 *   pred_out       optional uint8 (n, H, W)
 * One launch; the histogram is integer (LDS atomics, one 64-bit atomic per non-empty bin): the same input gives the same bits, and
 * a sample's prediction does not depend on the rest of its batch. A NULL descriptor, k outside 1..16, c outside 1..64, any of n, H,
 * W, h[i], w[i] below 1, a NULL logits[i], cm without labels, neither cm nor pred_out, an unknown label_dtype with labels, or more
 * than 2^31 - 1 output pixels return CMS_EINVAL, decided before any HIP call; nothing is launched. */
#define CMS_TTA_MAX_VIEWS 16
typedef struct {
    const float* logits[CMS_TTA_MAX_VIEWS];
    int h[CMS_TTA_MAX_VIEWS], w[CMS_TTA_MAX_VIEWS], flip[CMS_TTA_MAX_VIEWS];
    int n, c, H, W, k, align_corners;
    const void* labels;
    int label_dtype;      /* CMS_LABEL_U8 / CMS_LABEL_I64 */
    int ignore_index;
    int64_t* cm;
    uint8_t* pred_out;
} cms_tta_desc;
int cms_tta_resize(const void* src, void* dst, int n, int c, int H, int W, int Hs, int Ws, int dtype, int flip, void* stream);
int cms_tta_vote(const cms_tta_desc* d, void* stream);

/* Calibration and pseudo-label quality (csrc/calib.hip): the vote of cms_tta_vote with the confidence kept. One launch per batch
 * takes the place of the vote launch and ADDS exact integers into device-side tables; the reference has nothing of the kind.
 * A pixel is scored when its label is valid (label != ignore_index, 0 <= label < c), cms_tta_vote's rule. With inv_t = 1.0f / temps[t]
 * (one fp32 division on the host) and u_ic = v_ic * inv_t (v_ic as in cms_tta_vote; the multiply is skipped when temps[t] == 1):
 *   k >= 2   score_c = ((p_0c + p_1c) + ...), p_i = softmax(u_i) as in cms_tta_vote; pred the first index of the largest score;
 *            pbar_c = score_c / k; conf = min(pbar_pred, 1); nll = -logf(max(pbar_label, FLT_MIN)). At temps[0] == 1 pred is
 *            cms_tta_vote's bit for bit
 *   k == 1   pred the argmax of the logits v_0 exactly as cms_tta_vote takes it (any temperature); z = sum_c expf(u_c - max u),
 *            conf = 1 / z, pbar_c = expf(u_c - max u) * conf, nll = -((u_label - max u) - logf(z)). At temps[0] == 1 conf is the
 *            float the consistency kernels compare with conf_thresh and nll the cross-entropy kernels' per-pixel loss
 *   bin      #{ j : edges[j] <= conf }, an fp32 compare: nb bins from nb - 1 strictly ascending interior edges in (0, 1)
 *   hist     int64 (c, nb, 3), keyed by pred: += pixels, pixels with pred == label, sum of rint(conf * 2^24); temps[0]
 *   scores   int64 (2 + nt): += scored pixels, sum of rint(2^24 * sum_c (pbar_c - [c == label])^2) at temps[0], then per
 *            temperature t sum of rint(2^20 * min(nll_t, 88))
 *   cm, pred_out   as cms_tta_desc's, cm over the same scored pixels
 *   edges, temps   HOST memory (they travel as kernel arguments); every other pointer is device memory
 * Every sum is of integers, so it does not depend on the order of the atomics: the same input gives the same bits. Ranges: conf
 * <= 1, the squared error <= 2 and nll <= 88 give at most 2^31 * 88 * 2^20 < 2^58 per launch. The workgroup's tables live in LDS
 * (at most 64 KiB of scores, 48 KiB of histogram, 16 KiB of matrix) and leave with one 64-bit atomic per non-empty cell. Everything
 * cms_tta_vote refuses is refused, and: nb outside 1..48, edges NULL with nb > 1, an edge that is not in (0, 1) or not above
 * its predecessor, nt outside 1..8, temps NULL, a temperature that is not finite and > 0, hist / scores / labels NULL: CMS_EINVAL,
 * decided before any HIP call; nothing is launched. */
#define CMS_CALIB_MAX_BINS 48
#define CMS_CALIB_MAX_TEMPS 8
typedef struct {
    const float* logits[CMS_TTA_MAX_VIEWS];
    int h[CMS_TTA_MAX_VIEWS], w[CMS_TTA_MAX_VIEWS], flip[CMS_TTA_MAX_VIEWS];
    int n, c, H, W, k, align_corners;
    const void* labels;
    int label_dtype;      /* CMS_LABEL_U8 / CMS_LABEL_I64 */
    int ignore_index;
    int64_t* cm;
    uint8_t* pred_out;
    int nb;
    const float* edges;   /* nb - 1, host memory */
    int nt;
    const float* temps;   /* nt, host memory; temps[0] is the histogram's */
    int64_t* hist;
    int64_t* scores;
} cms_calib_desc;
int cms_calib_accumulate(const cms_calib_desc* d, void* stream);

/* ClassMix (csrc/classmix.hip; Olsson et al., WACV 2021): a mixing mask cut along the predicted class regions of a batch. Per
 * sample, with pred(y, x) the argmax over c of the bilinear sample (under `align_corners`) of logits[n, c] -- bit for bit the
 * prediction cms_tta_vote writes for k == 1 without a flip: first index on a tie, NaN maximal, no interpolation when (h, w) == (H, W):
 *   present        64-bit set, bit c set iff some pixel with valid != 0 has pred == c (every pixel when valid is NULL)
 *   chosen         the (popcount(present) + 1) / 2 classes of `present` that come first in the order (keys[n, c], c): ascending
 *                  key, the class index breaking equal keys; empty when present is
 *   mask_out       1.0f where valid != 0 and pred is in chosen, else 0.0f
 *   logits         (n, c, h, w) f32
 *   valid          optional (n, H, W) f32
 *   keys           (n, c) double, device memory; finite (NaN keys are outside the contract)
 *   mask_out       (n, H, W) f32
 *   pred_out       optional (n, H, W) uint8
 *   present_out, chosen_out   optional (n) uint64
 *   workspace      cms_classmix_workspace_bytes(n, H, W) bytes of device memory, 16-byte aligned, need not be initialised; that
 *                  function returns 0 for sizes cms_classmix refuses
 * Two stream-ordered launches, no atomics, no memset, no allocation and no host synchronisation: the same input gives the same bits
 * whatever the workspace held, a sample's mask does not depend on the rest of its batch, and the call can be captured in a graph.
 * A NULL descriptor, NULL logits / keys / mask_out / workspace, c outside 1..64, any of n, h, w, H, W below 1, more than 65535
 * samples, more than 2^31 - 1 output pixels or logits, or a workspace that is misaligned or too small return CMS_EINVAL, decided
 * before any HIP call; nothing is launched. */
typedef struct {
    const float* logits;
    const float* valid;
    const double* keys;
    int n, c, h, w, H, W, align_corners;
    float* mask_out;
    uint8_t* pred_out;
    uint64_t* present_out;
    uint64_t* chosen_out;
    void* workspace;
    size_t workspace_bytes;
} cms_classmix_desc;
size_t cms_classmix_workspace_bytes(int n, int H, int W);
int cms_classmix(const cms_classmix_desc* d, void* stream);

/* Cross pseudo supervision (csrc/cps.hip; Chen et al., CVPR 2021): the hard pseudo-labels two networks a and b give each other on a
 * CutMix-ed pair. Per output pixel (y, x) of sample n, for k = a, b:
 *   m            "take image 1": the bit the consistency kernels read from `ranges` under `invert`, or mask >= 0.5
 *   u_k(c)       the bilinear sample (under `align_corners`) of l1_k[n, c] if m, else of l0_k[n, c]; no interpolation when
 *                (h, w) == (H, W)
 *   pred_k       argmax over c of u_k(c): first index on a tie, NaN maximal -- with a constant mask, cms_tta_vote's single-view prediction
 *   conf_k       the largest softmax probability of u_k
 *   valid        um1 >= 0.5 if m, else um0 >= 0.5; a NULL map is all valid
 *   label_k      pred_k if valid and (conf_thresh <= 0 or conf_k >= conf_thresh), else 255
 *   stats        int64 [4]: valid pixels, labels != 255 in label_a, the same in label_b, valid pixels with pred_a == pred_b
 *   l0_a, l1_a, l0_b, l1_b   (n, c, h, w) f32
 *   ranges       (n, n_boxes, 4) int32 half-open [y0, y1, x0, x1], or NULL
 *   mask         (n, H, W) f32, or NULL: exactly one of ranges / mask
 *   um0, um1     optional (n, H, W) f32
 *   label_a, label_b   (n, H, W) uint8, every element written; stats: 8-byte aligned, need not be initialised
 * A 32-byte memset of stats and one launch on `stream`: no workspace, no allocation, no host synchronisation. The counts are
 * integer atomics: the same input gives the same bits whatever the outputs held, and a sample's labels do not depend on the rest of
 * its batch. A NULL descriptor, NULL logits / label_a / label_b / stats, c outside 1..64, any of n, h, w, H, W below 1, more than
 * 65535 samples, h > H or w > W, more than 2^31 - 1 output pixels, logits or range entries, both or neither of ranges / mask, ranges
 * with n_boxes < 1, or a misaligned stats return CMS_EINVAL, decided before any HIP call; nothing is launched. */
typedef struct {
    const float* l0_a;
    const float* l1_a;
    const float* l0_b;
    const float* l1_b;
    const int32_t* ranges;
    const float* mask;
    const float* um0;
    const float* um1;
    int n, c, h, w, H, W, align_corners, n_boxes, invert;
    float conf_thresh;
    uint8_t* label_a;
    uint8_t* label_b;
    int64_t* stats;
} cms_cps_desc;
int cms_cps_labels(const cms_cps_desc* d, void* stream);

/* Boundary IoU (Cheng et al., CVPR 2021) and trimap IoU (the DeepLab papers) as exact integer counts (csrc/boundary.hip). With
 * T = truth and P = pred with every void pixel (truth == ignore_index) set to ignore_index:
 *   D_M(p)         for a non-void pixel p of map M, the Chebyshev distance to the nearest position q that lies outside the h x w
 *                  array or has M(q) != M(p) (a void q is different); D >= 1, 1 on the array's edge. Stored as min(D, 255), 0 at
 *                  void pixels. D_M <= d is exactly G & ~erode^d(G) of the class mask G = (M == c): d 3 x 3 erosions, zero border
 *   bcm[j]         (c+1, c+1): with d = widths[i][j] clamped to 1..254, every non-void pixel of sample i whose T and P are classes
 *                  (< c) adds 1 at [D_T <= d ? T : c, D_P <= d ? P : c]; Boundary IoU of class a is
 *                  bcm[a][a] / (row a + column a - bcm[a][a]), the sums over all c + 1 entries
 *   tcm[j]         (c, c): every such pixel with D_T <= d adds 1 at [T, P]; trimap IoU is diag / (row + column - diag)
 *   truth, pred    (n, h, w) uint8
 *   widths         (n, k) int32, device memory; needed with bcm or tcm
 *   ignore_index   < 0: no pixel is void
 *   bcm, tcm       optional int64 (k, c+1, c+1) / (k, c, c), accumulated into
 *   dist_truth, dist_pred   optional (n, h, w) uint8, receive the stored D_T / D_P
 *   workspace      cms_boundary_workspace_bytes(n, h, w) bytes of device memory, 16-byte aligned, need not be initialised; that
 *                  function returns 0 for sizes cms_boundary_confusion refuses
 * Stream-ordered launches whose number depends on c and k only (a row pass, a column pass, ceil(k / fit) counting passes with fit
 * the widths whose histograms fit 64 KiB of LDS), no allocation and no host synchronisation; the workspace is six bytes per pixel. Integer atomics: the same input gives
 * the same bits. No window crosses from one sample of the batch into the next, and label 255 round an image counts as the outside
 * of the array does, so an image's counts do not depend on its batch or on the canvas it is padded to. A NULL descriptor, NULL
 * truth / pred / workspace, NULL widths with bcm or tcm, nothing to produce (bcm, tcm and both distance outputs NULL), k outside
 * 1..4, num_classes outside 1..64, any of n, h, w below 1, more than 2^31 - 1 pixels, or a workspace that is misaligned or too
 * small return CMS_EINVAL, decided before any HIP call; nothing is launched. */
typedef struct {
    const uint8_t* truth;
    const uint8_t* pred;
    const int32_t* widths;
    int n, h, w, num_classes, ignore_index, k;
    int64_t* bcm;
    int64_t* tcm;
    uint8_t* dist_truth;
    uint8_t* dist_pred;
    void* workspace;
    size_t workspace_bytes;
} cms_boundary_desc;
size_t cms_boundary_workspace_bytes(int n, int h, int w);
int cms_boundary_confusion(const cms_boundary_desc* d, void* stream);

/* CRF refinement of a prediction against its image (csrc/crf.hip). This project's own truncated form of the fully connected CRF of
 * Kraehenbuehl & Koltun (NIPS 2011) with the two DeepLab kernels, in the spirit of Convolutional CRFs (Teichmann & Cipolla, BMVC
 * 2018): mean-field inference with a Potts compatibility over a dilated square window, cut to each sample's rectangle. The reference
 * has nothing of the kind. Per pixel p of sample i:
 *   P(p, c)      cms_tta_vote's score of the k views for every k (k == 1: the softmax of the upsampled logits), divided by k;
 *                logP = log(max(P, FLT_MIN)), Q^0 = P. The unary prediction is the first index of the largest score
 *   W(p)         { p + dilation (dy, dx) : |dy|, |dx| <= radius, (dy, dx) != 0 } cut to the rectangle rect[i] = (top, left, h, w);
 *                n(p) = |W(p)|, an exact integer. Padding and pixels of another sample are never neighbours
 *   k(p, q)      [ bi_w exp(-|p-q|^2 / (2 bi_xy^2) - |I_p-I_q|^2 / (2 bi_rgb^2)) + pos_w exp(-|p-q|^2 / (2 pos_xy^2)) ] / n(p),
 *                I the rgb bytes as grey levels 0..255; divided by the neighbour COUNT, not the sum of the kernel values
 *   Q^{t+1}(p,.) softmax_c( logP(p, c) + sum over q in W(p) of k(p, q) Q^t(q, c) ), all pixels at once (Jacobi), t < iters;
 *                the sum runs over the window in row-major (dy, dx) order in fp32; no neighbour, no message
 *   pred         inside the rectangle the first index of the largest Q^iters, outside it the unary prediction
 *   logits, h, w, flip, n, c, H, W, k, align_corners, labels, label_dtype, ignore_index, cm   as cms_tta_desc's
 *   rgb          (n, 3, H, W) uint8, device memory
 *   rect         (n, 4) int32 in HOST memory: it is checked before anything is launched and travels as kernel arguments
 *   pred_out     optional uint8 (n, H, W); q_out optional f32 (n, c, H, W): Q^iters inside the rectangles, P outside
 *   stats        int64 [2], device memory, 8-byte aligned, need not be initialised: pixels inside rectangles, of those the
 *                pixels whose pred differs from the unary prediction
 *   workspace    cms_crf_workspace_bytes(n, c, H, W) bytes of device memory, 16-byte aligned, need not be initialised; that
 *                function returns 0 for sizes cms_crf_refine refuses
 * Per group of 32 samples one unary launch and `iters` mean-field launches on `stream` (ping-pong Q in the workspace; the last
 * one fuses argmax, histogram and counts), plus a 16-byte memset of stats; no allocation, no host synchronisation. The histogram
 * and counts are integer atomics: the same input gives the same bits, and given the same P and rgb a sample's result does not
 * depend on its batch, its canvas or its offset on it. A NULL descriptor, NULL logits[i] / rgb / rect / stats / workspace, k
 * outside 1..16, c outside 1..64, any of n, H, W, h[i], w[i] below 1, radius outside 1..5, dilation outside 1..16, iters outside
 * 1..32, a weight that is negative or not finite, a theta that is not finite and > 0, a rectangle that is empty or leaves the
 * canvas, cm without labels, nothing to produce, an unknown label_dtype with labels, more than 2^31 - 1 output pixels, a misaligned
 * stats, or a workspace that is misaligned or too small return CMS_EINVAL, decided before any HIP call; nothing is launched. */
typedef struct {
    const float* logits[CMS_TTA_MAX_VIEWS];
    int h[CMS_TTA_MAX_VIEWS], w[CMS_TTA_MAX_VIEWS], flip[CMS_TTA_MAX_VIEWS];
    int n, c, H, W, k, align_corners;
    const uint8_t* rgb;
    const int32_t* rect;
    int radius, dilation, iters;
    float bi_w, bi_xy, bi_rgb, pos_w, pos_xy;
    const void* labels;
    int label_dtype;      /* CMS_LABEL_U8 / CMS_LABEL_I64 */
    int ignore_index;
    int64_t* cm;
    uint8_t* pred_out;
    float* q_out;
    int64_t* stats;
} cms_crf_desc;
size_t cms_crf_workspace_bytes(int n, int c, int H, int W);
int cms_crf_refine(const cms_crf_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* Surface distances between a truth and a prediction map as exact integers (csrc/surface.hip): what the Hausdorff distance (HD,
 * Huttenlocher et al. 1993), its 95th percentile (HD95) and the average symmetric surface distance (ASSD) follow from, in MedPy's
 * convention with connectivity 1 and unit spacing. With T = truth and P = pred with every void pixel (truth == ignore_index) set
 * to void, per sample i and class c < num_classes, G = (T_i == c) and S = (P_i == c):
 *   surface        dM: the pixels of a mask M with at least one of their FOUR edge neighbours outside M; a neighbour outside the
 *                  h x w array, or a void one, is outside M (M & ~binary_erosion(M, cross, border_value=0)). Boundary IoU uses
 *                  the 3 x 3 neighbourhood; this does not
 *   d2(p, dG)      min over q in dG of (py - qy)^2 + (px - qx)^2, an exact integer < 2^30
 *   scored         the pair (i, c) when G and S are both non-empty
 *   stats          int64 (n, c, 6), written: [|dS|, |dG|, max d2(p, dG) over dS, max d2(q, dS) over dG, a[lo], a[hi]] with a the
 *                  sorted pooled multiset of all |dS| + |dG| = m squared distances, lo = 19 (m - 1) / 20 (integer division) and
 *                  hi = min(lo + 1, m - 1): numpy.percentile(sqrt(a), 95) is sqrt(a[lo]) + (19 (m - 1) % 20) / 20 * (sqrt(a[hi])
 *                  - sqrt(a[lo])). An unscored pair gets its two counts and -1 in the other four
 *   sums           double (n, c, 2), written: [sum over dS of sqrt(d2(p, dG)), sum over dG of sqrt(d2(q, dS))], 0.0 for an unscored
 *                  pair. Summed in a fixed order without atomics: the same input gives the same bits
 *   d2_pred, d2_truth   optional int32 (n, h, w): d2 at every surface pixel of a scored pair (dS / dG), -1 everywhere else
 *   truth, pred    (n, h, w) uint8;  ignore_index < 0: no pixel is void
 *   workspace      cms_surface_workspace_bytes(n, h, w, num_classes) bytes of device memory, 16-byte aligned, need not be
 *                  initialised; that function returns 0 for sizes cms_surface_distances refuses
 * A fixed number of stream-ordered launches (one memset, mark, rows, column walk, and with stats or sums a reduction and four
 * radix-select passes), no allocation, no host synchronisation, no float atomics. Distances are between pixels of one sample only,
 * and label 255 round an image counts as the outside of the array does, so a sample's numbers do not depend on its batch or on the
 * canvas it is padded to. A NULL descriptor, NULL truth / pred / workspace, nothing to produce (stats, sums and both maps NULL),
 * num_classes outside 1..64, any of n, h, w below 1, h or w above 16384, 2^31 pixels or more, or a workspace that is misaligned or
 * too small return CMS_EINVAL, decided before any HIP call; nothing is launched. */
typedef struct {
    const uint8_t* truth;
    const uint8_t* pred;
    int n, h, w, num_classes, ignore_index;
    int64_t* stats;
    double* sums;
    int32_t* d2_pred;
    int32_t* d2_truth;
    void* workspace;
    size_t workspace_bytes;
} cms_surface_desc;
size_t cms_surface_workspace_bytes(int n, int h, int w, int num_classes);
int cms_surface_distances(const cms_surface_desc* d, void* stream);

/* Sliding-window evaluation (csrc/window.hip): every view of an evaluation batch is covered by overlapping windows of one size, the
 * network sees the windows, and one launch stitches the windows' low-resolution logits into the prediction of the canvas. The
 * reference evaluates whole images; the definition below is this project's own.
 *
 * The canvas is H x W; view v has size (Hv, Wv) and may be mirrored. The window is (wh, ww), a view's stride (sh, sw). Per view and
 * axis (y shown, x alike):
 *   eh      min(wh, Hv), the effective window height
 *   gy      1 if Hv <= wh, else ceil((Hv - wh) / sh) + 1 windows
 *   y1_j    min(j * sh, Hv - eh), j < gy: the last window is flush with the edge
 *   G       gy * gx windows, all (eh, ew); window (j, i) of sample n is item (n * gy + j) * gx + i of the view's window batch, whose
 *           logits are (n * G, c, hl, wl) f32
 *
 * cms_window_crop: all windows of one view in one launch, straight from the canvas image.
 *   src     (n, c, H, W), dst (n * G, c, eh, ew), both of `dtype` (CMS_F32 / CMS_BF16), dense; must not overlap
 *   dst[(n * gy + j) * gx + i, ch, y, x] is bit for bit element (n, ch, y1_j + y, x1_i + x) of what cms_tta_resize makes of src at
 *           (Hv, Wv) with `flip`; the view is never materialised. With (Hv, Wv) == (H, W) and no flip it is a strided copy. Every
 *           element of dst is written.
 * NULL pointers, a size below 1, an unknown dtype, a stride above its window or below ceil(window / 4), or more than 2^31 - 1
 * elements in src or dst return CMS_EINVAL, decided before any HIP call.
 *
 * cms_window_vote: per canvas pixel (y, x) of sample n, for view v in order:
 *   G == 1  the view is read exactly as cms_tta_vote reads a view of (hl, wl): same taps, same un-mirroring, same softmax;
 *           score_c += p_c
 *   G > 1   the pixel's view row is ry = min(Hv - 1, ((2 y + 1) Hv) / (2 H)) in integers (ry = y when Hv == H), its column rx
 *           alike and then, for a mirrored view, rx = Wv - 1 - rx. The covering windows are those with y1_j <= ry < y1_j + eh and
 *           x1_i <= rx < x1_i + ew, cnt their number (>= 1). For each covering window in row-major (j, i) order the taps are
 *           bilin_tap(ry - y1_j, bilin_scale(hl, eh, align_corners), hl, align_corners), x alike and never mirrored (the
 *           coordinate already is); the window's logits are gathered at them, p = softmax as in cms_tta_vote, and
 *           score_c += p_c / (float)cnt (one fp32 division per class and window)
 *   pred    the first index of the largest score, NaN counting as maximal
 * If every view has G == 1 the call IS cms_tta_vote on (hl, wl, flip) -- its single-view argmax of the logits included. labels,
 * label_dtype, ignore_index, cm and pred_out are cms_tta_desc's. One launch, no workspace, no host synchronisation; integer
 * histogram: the same input gives the same bits, and a sample's prediction does not depend on the rest of its batch. Whatever
 * cms_tta_vote refuses (with h = hl, w = wl), Hv or Wv below 1, a window or stride below 1, a stride above its window or below
 * ceil(window / 4), eh / ew / gy / gx that do not follow from (Hv, Wv, window, stride), hl > eh or wl > ew, or more than 2^31 - 1
 * logits in a view return CMS_EINVAL, decided before any HIP call; nothing is launched. */
typedef struct {
    const float* logits[CMS_TTA_MAX_VIEWS];
    int hl[CMS_TTA_MAX_VIEWS], wl[CMS_TTA_MAX_VIEWS], Hv[CMS_TTA_MAX_VIEWS], Wv[CMS_TTA_MAX_VIEWS];
    int gy[CMS_TTA_MAX_VIEWS], gx[CMS_TTA_MAX_VIEWS], eh[CMS_TTA_MAX_VIEWS], ew[CMS_TTA_MAX_VIEWS];
    int sh[CMS_TTA_MAX_VIEWS], sw[CMS_TTA_MAX_VIEWS], flip[CMS_TTA_MAX_VIEWS];
    int wh, ww;           /* the window */
    int n, c, H, W, k, align_corners;
    const void* labels;
    int label_dtype;      /* CMS_LABEL_U8 / CMS_LABEL_I64 */
    int ignore_index;
    int64_t* cm;
    uint8_t* pred_out;
} cms_window_desc;
int cms_window_crop(const void* src, void* dst, int n, int c, int H, int W, int Hv, int Wv, int flip, int wh, int ww, int sh, int sw,
                    int dtype, void* stream);
int cms_window_vote(const cms_window_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CUTMIXSEG_H */

/* libsegengine — C-ABI of the MI355X (gfx950) segmentation engine.
 *
 * Drop-in boundary for the hot path of junqiangchen/PytorchDeepLearing.  The
 * reference has no FFI of its own — its boundary is Python duck typing — so every entry point
 * cites the reference interface it stands behind.  Plain pointers and sizes only; no torch types.
 *
 * Ownership: the caller allocates and owns every buffer (parameters, gradients, optimiser state,
 * workspace, inputs, outputs); the engine keeps views plus small host-side descriptors.
 * Errors: every function returns 0 on success, <0 on failure; seg_last_error() gives the message.
 * Threading: calls are stream-ordered and asynchronous; a handle is not thread-safe.
 * All device pointers must be 256-byte aligned.  `stream` is a hipStream_t.
 *
 * Environment switches read by the PRODUCT library (each selects a complete path that the parity tests cover; none is needed to run; read once per
 * process unless noted) - the whole list:
 *   SEG_WGRAD_STREAM=0   weight gradients on the caller's stream instead of the library's second (low-priority) stream
 *   SEG_CONV3X=0         16-bit halo convolutions through conv3_kernel (round 1) instead of c3x::conv3x_kernel - bit-identical results
 *   SEG_STEMX=0          separate image-stem / GroupNorm / stem weight-gradient kernels instead of the fused input block
 *   SEG_STEMX_ONEPASS=0|2 (read per seg_create) backward of the fused input block: 0 = two passes over the gradient sources (reduce; apply + stem weight
 *                        gradients); otherwise ONE pass collects the GroupNorm sums and the coefficient-free moments of the stem weight gradients, and a
 *                        combine launch behind the finalize applies the coefficients in fp64 - default where a gradient source is >= 16 MB, 2 = at every size
 *   SEG_VHEAD=0          the head writes its data-gradient tensor instead of the on-the-fly form
 *   SEG_GN_FOLD=0        GroupNorm finalize as launches of its own;  SEG_DUAL_GN=0: one GroupNorm-backward pass per branch of the VNet input block
 *   SEG_GN_COOP=0        (read per seg_create) GroupNorm backward of the >= 64-channel levels as reduce + apply launches instead of the one-launch
 *                        kernel whose workgroups exchange their partial sums inside the launch
 *   SEG_HEAD_FUSE=0      (read per seg_create) the 1^d head (networks/VNet3d.py:83-99) as a launch of its own instead of inside the activation pass that produces its
 *                        input (bit-identical results)
 *   SEG_HEAD_WFUSE=0|2   (read per seg_create) weight / bias gradient of a ONE-class head: 0 = head_bwd_kernel reads the head's input; otherwise the
 *                        GroupNorm-backward reduce passes of the units that input is made of collect it (they hold dlogits and the activations already) and
 *                        seg_train_step does not write the head's input at all - default on tensors >= 16 MB, 2 = at every size.  Other heads: no effect
 *   SEG_RQ_FUSE=0        (read per seg_create) the GroupNorm-backward reduction of a VNet up-conv unit as a launch of its own instead of riding on the
 *                        data-gradient launch of the 1^d conv that produces its gradient
 *   SEG_VACT=0|2         (read per seg_create) the activation between a VNet up-conv and the 1^d conv on the concat (networks/VNet3d.py:72-77): 0 = written as a
 *                        tensor at every level, 2 = applied by its two readers on load at every level the kernels allow (default: on tensors >= 16 MB) -
 *                        bit-identical results
 *   SEG_STEP_RIDERS=0    (read per step) step counters / flag clears as launches of their own instead of riding on neighbouring kernels
 *   SEG_PACK_SPLIT=0     the weight re-layout as one launch on the caller's stream
 *   SEG_CONV_STREAM=0    the generic implicit-GEMM kernel also where the register-resident streaming conv applies
 *   SEG_WG_DIRECT=0      1^d-conv weight gradients through wgrad_kernel instead of the multi-step streaming kernel
 *   SEG_WG_S2=0|2        (read per launch) weight gradients of the 2^d stride-2 windows on 16-bit tensors (down-convolutions, ConvTranspose up-convolutions;
 *                        fine extents twice the coarse ones, 32 x 16 tile): 0 = wgrad_kernel, 2 = the multi-step streaming wgrad_s2_kernel on wgrad_kernel's
 *                        voxel slices (bit-identical results), default = wgrad_s2_kernel on fewer, longer slices (other order of the fp32 slice sums)
 *   SEG_W3_BOX16=0|2    the 4 x 8 x 16-box weight gradient of the 16-channel level: off / forced onto small volumes (operator tests)
 *   SEG_C3X_MAP="cin:cout:w=id,..."   per-shape halo-conv tiling override (tools/tune_conv3x.py)
 *   SEG_C3X16_REUSE=0    the 16 -> 16 channel 3-D halo convs through conv3x16_kernel (one LDS fragment read per MFMA, weight layout 2) instead of
 *                        conv3x16r_kernel (fragments reused across the kh taps, weight layout 3) - bit-identical on integer data
 * The tuning knobs and measured-slower paths of rounds 1-5 (double-buffered weight gradient, GroupNorm in the consumer conv, persistent halo convs, flag
 * forks, sub-batched levels, second weight-gradient stream) were removed from the sources in round 6; what each measured is in profiles/HISTORY.md.
 */
#ifndef SEGENGINE_H
#define SEGENGINE_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct seg_engine* seg_handle;

enum { SEG_NET_VNET = 0, SEG_NET_UNET = 1, SEG_NET_RESNET = 2 };
enum { SEG_F32 = 0, SEG_F16 = 1, SEG_BF16 = 2 };
enum { SEG_LABEL_U8 = 0, SEG_LABEL_I32 = 1, SEG_LABEL_I64 = 2, SEG_LABEL_F32 = 3,
       /* flag, or-ed into a label type: every kernel reads the label as (value != 0): `y[y != 0] = 1` of the binary training loops
        * (model/modelVNet.py:576) on the device, so e.g. 0/255 mask images go to the loss / metric / clDice kernels as stored */
       SEG_LABEL_BINARIZE = 16 };
/* loss_name strings of model/modelVNet.py:68-76,513-521,750-756 */
enum {
    SEG_LOSS_BINARY_DICE = 0,     /* model/losses.py:33-53   BinaryDiceLoss */
    SEG_LOSS_BINARY_CE = 1,       /* model/losses.py:129-147 BinaryCrossEntropyLoss */
    SEG_LOSS_BINARY_FOCAL = 2,    /* model/losses.py:150-181 BinaryFocalLoss */
    SEG_LOSS_BINARY_CE_DICE = 3,  /* model/losses.py:184-197 BinaryCrossEntropyDiceLoss */
    SEG_LOSS_MULTI_CE = 4,        /* model/losses.py:247-260 MutilCrossEntropyLoss */
    SEG_LOSS_MULTI_FOCAL = 5,     /* model/losses.py:263-285 MutilFocalLoss */
    SEG_LOSS_MULTI_DICE = 6,      /* model/losses.py:288-325 MutilDiceLoss */
    /* not selectable through the reference wrappers' loss_name; same reduction, other ratios */
    SEG_LOSS_BINARY_JACCARD = 7,  /* model/losses.py:9-30    BinaryJaccardLoss */
    SEG_LOSS_BINARY_ELDICE = 8,   /* model/losses.py:56-74   BinaryELDiceLoss */
    SEG_LOSS_BINARY_TVERSKY = 9,  /* model/losses.py:102-126 BinaryTverskyLoss (alpha 0.3, beta 0.7) */
    SEG_LOSS_MULTI_CE_DICE = 10,  /* model/losses.py:328-342 MutilCrossEntropyDiceLoss */
    SEG_LOSS_MULTI_ELDICE = 11,   /* model/losses.py:345-382 MutilELDiceLoss */
    SEG_LOSS_BINARY_SS = 12,      /* model/losses.py:77-99   BinarySSLoss (sensitivity-specificity, r = 0.1) */
    SEG_LOSS_MULTI_TVERSKY = 13,  /* model/losses.py:421-459 MutilTverskyLoss: class_alpha = its alpha tensor (class weight AND false-positive weight);
                                     beta (never defined by the class; set by the caller) is passed in the focal_gamma argument */
    SEG_LOSS_MULTI_SS = 14,       /* model/losses.py:385-418 MutilSSLoss: r (never defined by the class) is passed in the focal_gamma argument */
    SEG_LOSS_BINARY_MCC = 15      /* model/losses.py:200-232 MCC_Loss: the `logits` argument holds PROBABILITIES (its `inputs`), dlogits = d loss / d inputs;
                                     torch.add(a, 1, b) read as a + 1*b (the torch 1.x signature the reference was written for) */
};
enum { SEG_MASKS_EVAL = 0, SEG_MASKS_GIVEN = 1, SEG_MASKS_RANDOM = 2 };

/* networks/VNet3d.py:109 VNet3d(image_channel, numclass, init_features=16), networks/VNet2d.py:109,
 * networks/Unet3d.py:11 UNet3d(in_channels, out_channels, init_features=16), networks/Unet2d.py:11.
 * ndim = 2 or 3.  in_channels 1..16 (1 in 3-D / 1..3 in 2-D take the fused image stem; more channels are zero-padded to a 16-channel image tensor
 * and run through the ordinary 16-channel convs), num_class 1..16, init_features 16.
 *
 * SEG_NET_RESNET: the classifiers networks/ResNet3d.py:72-118 / ResNet2d.py ResNet3d(image_channel, numclass) - the VNet encoder (in_tr, down_tr32 ..
 * down_tr256), global average pooling, Linear(256, 128) + ReLU + Linear(128, numclass).  70 parameter tensors in state_dict order, the last four
 * fc_layers.0.weight [128][256], fc_layers.0.bias, fc_layers.2.weight [numclass][128], fc_layers.2.bias.  Channel dropout sits only behind each down_conv
 * (4 calls of 32, 64, 128, 256 channels; the input block and the LUConvs have none and take multiplier 1 in every mask mode).  The reference reads an
 * undefined module global `prob` for the dropout probability and cannot be constructed as shipped; p = 0.2, the VNet value, is used.
 * For this kind `logits` / `probs` / `dlogits` are [N][num_class] fp32 (the planar layout with one voxel): probs = sigmoid for num_class == 1, soft-max
 * over the classes otherwise.  seg_forward, seg_backward*, seg_train_step and the captured step work as for the other kinds; the losses of
 * seg_train_step are evaluated with v = 1 (SEG_LOSS_BINARY_CE, BINARY_FOCAL, MULTI_CE, MULTI_FOCAL are the reference's choices), and out3[1..2]
 * (dice / iou of a one-voxel "mask") are written but carry no meaning. */
int seg_create(int net_kind, int ndim, int in_channels, int num_class, int init_features, int dtype,
               seg_handle* out);
void seg_destroy(seg_handle h);

/* Parameter table in reference state_dict order: name, PyTorch shape, and the
 * offset (in floats) of the tensor inside the flat fp32 parameter / gradient buffers. */
int seg_param_count(seg_handle h);
int seg_param_info(seg_handle h, int index, char* name, int name_cap, int* shape8, int* ndim,
                   long long* offset);
long long seg_param_numel(seg_handle h);

/* Number of channel-dropout calls per forward (34 VNet / 18 UNet / 4 ResNet) and the row stride of the
 * multiplier table [calls][N][ld] used by SEG_MASKS_GIVEN (networks/VNet3d.py:11,31,51,67). */
int seg_dropout_calls(seg_handle h);
int seg_dropout_ld(seg_handle h);
int seg_dropout_channels(seg_handle h, int call);

/* SEG_MASKS_RANDOM forwards issued so far (the mask of draw k is a function of (seed, k)); a resumed run restores it so that the mask
 * sequence continues instead of restarting (torch's generator state in the reference, model/modelVNet.py:570-596 under nn.Dropout3d). */
long long seg_dropout_draws(seg_handle h);
int seg_set_dropout_draws(seg_handle h, long long draws);

/* Fix the batch shape (N, D, H, W; D ignored for ndim 2) and size the workspace. */
int seg_plan(seg_handle h, int n, int d, int hgt, int wid);
long long seg_workspace_bytes(seg_handle h);
/* what the planner decided for the current shape (tests / diagnostics): what = 1: convolution units, 2: fork events the last backward pass recorded
 * on the caller's stream, 3: 1 where the head's weight gradient comes out of the GroupNorm-backward reduce passes (SEG_HEAD_WFUSE), else 0, 4: 1 where the backward of the fused
 * input block reads its gradient sources once (SEG_STEMX_ONEPASS), else 0.
 * <0: not planned / unknown `what`. */
int seg_plan_count(seg_handle h, int what);

/* Bind caller-owned buffers: flat fp32 params / grads (seg_param_numel floats each) + workspace. */
int seg_bind(seg_handle h, float* params, float* grads, void* workspace);

/* Re-layout the fp32 master weights into the run-dtype GEMM layouts (call after every update). */
int seg_pack_weights(seg_handle h, void* stream);

/* forward(x) -> (logits, probs): x is fp32 NC[D]HW like the reference datasets deliver
 * (model/dataset.py:107), logits/probs are fp32 NC[D]HW (networks/VNet3d.py:90-99,129-158).
 * mask_mode: SEG_MASKS_EVAL = model.eval(); SEG_MASKS_GIVEN = `masks` holds the per-call (n,c)
 * dropout multipliers; SEG_MASKS_RANDOM = engine draws them from (seed, internal step). */
int seg_forward(seg_handle h, const float* x, int mask_mode, const float* masks,
                unsigned long long seed, float* logits, float* probs, void* stream);

/* backward of the last forward given d(loss)/d(logits) (fp32 NC[D]HW, already multiplied by
 * seg_get_loss_scale); parameter gradients (times the loss scale) are ACCUMULATED into the bound
 * flat gradient buffer (zero_grads != 0 clears it first — `opt.zero_grad()` of
 * model/modelVNet.py:593). */
int seg_backward(seg_handle h, const float* dlogits, int zero_grads, void* stream);
/* Bucketed gradient exchange (one process per GPU): the backward pass is a fixed list of seg_backward_ops() operations.
 * seg_backward_bucket finds the earliest op count `op_split` after which a suffix [param_offset, numel) of the flat gradient
 * buffer holding at least `tail_fraction` of the elements is final (gradients finish in reverse registration order);
 * seg_backward_range runs ops [op_begin, op_end) and joins the weight-gradient side stream, so the caller can start the
 * collective on that suffix while the remaining ops run.  seg_backward == seg_backward_range(0, seg_backward_ops()). */
int seg_backward_ops(seg_handle h);
int seg_backward_bucket(seg_handle h, double tail_fraction, int* op_split, long long* param_offset);
int seg_backward_range(seg_handle h, const float* dlogits, int zero_grads, int op_begin, int op_end, void* stream);
/* the same with join = 0: the slice's weight gradients are released to the engine's side stream but `stream` does not wait for them;
 * seg_side_wait(other_stream) makes ANOTHER stream (the one a collective is ordered after) wait for every weight gradient issued so far, so the
 * backward pass itself never stalls at a bucket boundary.  The last slice of a pass must be run with join = 1 (or through seg_backward_range). */
int seg_backward_slice(seg_handle h, const float* dlogits, int zero_grads, int op_begin, int op_end, int join, void* stream);
int seg_side_wait(seg_handle h, void* stream);

/* ---- feature taps: the output of a named module as the passes left it in the workspace (what a forward / backward hook on that module would see).
 * Taps of this version: "in_tr", "down_tr32", "down_tr64", "down_tr128", "down_tr256" - the input block and the four DownTransitions of the encoder that
 * SEG_NET_VNET and SEG_NET_RESNET share (networks/VNet3d.py:25-59, ResNet3d.py:24-58) - and, SEG_NET_VNET only, "up_tr32": the last UpTransition, the head's
 * input (its gradient is virtual under a one-class head); SEG_NET_UNET has none, and any other name is "not found".
 * seg_feature_find: the tap's id (>= 0; valid for the life of the handle), its channels and its level (extents = input extents >> level); < 0 and
 * seg_last_error() for an unknown name.
 * seg_feature_read: out = the activation as fp32 NC[D]HW (n * channels * voxels floats of device memory); want_grad != 0: d(what the caller seeded the
 * backward pass with) / d(that activation) instead - the contribution tensors of the tap summed in fp32 in the order the backward pass wrote them (a VNet
 * skip level has two), divided by the handle's loss scale (dlogits are handed to seg_backward times that scale).
 * Validity is tracked by the handle: the activation is readable after a seg_forward at the current plan, the gradient after a COMPLETE backward pass of
 * that forward (seg_backward, or every slice of the op list in order).  seg_plan, seg_bind, seg_train_step and seg_train_graph_launch leave nothing to
 * read, and a seg_set_loss_scale that changes the scale leaves no gradient (the tensors carry the old one); every such call fails with a message that names what is missing, as does a contribution that is never written (virtual).
 * Nothing here changes the plan: no workspace byte, no op of the forward or backward lists. */
int seg_feature_find(seg_handle h, const char* name, int* channels, int* level);
int seg_feature_read(seg_handle h, int id, int want_grad, float* out, void* stream);
/* Grad-CAM (model/visualization.py:112-238 of the reference) of nlayers (1..16) taps from the tensors of the last forward and backward pass (validity as
 * for seg_feature_read with want_grad): per layer the map of seg_op_gradcam below with weight 1 / nlayers, accumulated in `out` in the order of `ids`,
 * finalized after the last.  out: fp32 [N][D]HW at the input resolution, values in [0, 1].  For the reference's map the backward pass is seeded with
 * dlogits = loss scale at [n][target class of sample n], 0 elsewhere.  ws: seg_gradcam_ws_bytes() bytes (any nlayers: the layers share it), 256-byte
 * aligned; no allocation, no host synchronisation, two calls on the same tensors agree bit for bit. */
long long seg_gradcam_ws_bytes(seg_handle h, int nlayers);
int seg_gradcam(seg_handle h, const int* ids, int nlayers, void* ws, float* out, void* stream);

int seg_set_loss_scale(seg_handle h, float scale);
float seg_get_loss_scale(seg_handle h);

/* Losses and metrics on planar fp32 logits [N][C][V] (model/losses.py, model/metric.py:146-215).
 * out3 = {loss, dice metric, iou metric}.  `ws` needs seg_loss_ws_bytes(N, C) bytes; it carries
 * the reduction results from seg_loss_forward to seg_loss_backward. */
long long seg_loss_ws_bytes(int n, int c);
int seg_loss_forward(const float* logits, const void* target, int label_type, int n, int c,
                     long long v, int loss_kind, float focal_alpha, float focal_gamma,
                     const float* class_alpha, void* ws, float* out3, void* stream);
int seg_loss_backward(const float* logits, const void* target, int label_type, int n, int c,
                      long long v, int loss_kind, float focal_alpha, float focal_gamma, void* ws,
                      float grad_scale, float* dlogits, void* stream);
/* Exact global-batch losses across data-parallel ranks (SURVEY.md section 8e mode ii).  The reference losses are
 * batch-global ratios (model/losses.py:50-51 BinaryDiceLoss sums over the whole batch; :315-325 MutilDiceLoss reduces
 * over dim (0,2) and counts the classes present in the batch; :259 the CE / focal means divide by the batch voxel
 * count), so a rank-local loss is NOT the loss of the global batch.  seg_loss_forward == seg_loss_reduce followed by
 * seg_loss_finalize(n_global = n).  Across ranks: seg_loss_reduce, SUM-all-reduce the first seg_loss_shared_doubles()
 * doubles of `ws` (I, sum p, sum y, sum bce/nll, sum focal, per-class I_c / P_c / Y_c), seg_loss_finalize with
 * n_global = samples over all ranks (or 0: the count is read on the device - seg_loss_reduce leaves the local sample count in double
 * [5] of `ws`, so the all-reduce of the shared doubles delivers the global count and unequal shards need no host read),
 * seg_loss_backward; parameter gradients are then SUMMED over ranks (not averaged).
 * The metrics in out3[1..2] stay per-rank (they are per-sample means, model/metric.py:146-155). */
int seg_loss_shared_doubles(void);
int seg_loss_reduce(const float* logits, const void* target, int label_type, int n, int c, long long v,
                    int loss_kind, float focal_alpha, float focal_gamma, void* ws, void* stream);
int seg_loss_finalize(const float* logits, const void* target, int label_type, int n, int c, long long v,
                      int loss_kind, float focal_alpha, float focal_gamma, const float* class_alpha,
                      int n_global, void* ws, float* out3, void* stream);
/* Lovasz losses (model/lovasz.py:20-141 through model/losses.py:235-242 BinaryLovaszLoss and :462-473 LovaszLoss; per_image = False, no
 * ignore index).  x: fp32 [n][c][v].  c == 1: Lovasz hinge on logits, target in {0,1}.  c > 1: the reference's LovaszLoss, which hands
 * its `logits` argument to _lovasz_softmax as class probabilities WITHOUT a soft-max - x is used as given (pass probabilities for the
 * published Lovasz-Softmax); classes = 'present', mean over the present classes.  One radix sort of n*v (error, index) pairs per class.
 * out1[0] = loss; dx [n][c][v] = d loss / d x (written by the forward pass - the backward is a scaling by the incoming gradient).
 * ws: seg_lovasz_ws_bytes(n, v) bytes.  n*v < 2^32. */
long long seg_lovasz_ws_bytes(int n, long long v);
int seg_lovasz_forward(const float* x, const void* target, int label_type, int n, int c, long long v, void* ws, float* out1, float* dx,
                       void* stream);
/* SSIM / SSIM3D (model/lossesSSIM.py:47-99, 102-167): img1, img2 fp32 [n][c][d][h][w] (nd = 2: d = 1), Gaussian window `window` (11 in the
 * reference, sigma 1.5), zero padding, the same window for every channel.  out[0] = mean of the SSIM map (size_average=True),
 * out[1 .. n] = the per-sample means.  seg_ssim_forward leaves the derivative maps in ws (seg_ssim_ws_bytes(n, c, d*h*w) bytes) for
 * seg_ssim_backward: dimg = gscale * d(sum of the map)/d img, gscale[0] (per_sample = 0), gscale[sample] (per_sample = 1) or gscale[sample][x] (per_sample = row length w >= 2) carrying the
 * incoming gradient times 1/count; dimg1 or dimg2 may be NULL.  The backward pass consumes ws (one backward per forward).
 * Limits: n <= 64, window odd and <= 15. */
long long seg_ssim_ws_bytes(int n, int c, long long v);
int seg_ssim_forward(const float* img1, const float* img2, int n, int c, int d, int h, int w, int nd, int window, void* ws, float* out,
                     void* stream);
/* the same forward pass, additionally out_cols[n][w] = the map's means over (c, d, h): what `ssim3D(size_average=False)` returns in the reference (its
 * `.mean(1).mean(1).mean(1)` of a 5-D map, model/lossesSSIM.py:92-97, leaves (N, W)); seg_ssim_backward takes the matching gscale[n][w] with per_sample = w */
int seg_ssim_forward_cols(const float* img1, const float* img2, int n, int c, int d, int h, int w, int nd, int window, void* ws, float* out,
                          float* out_cols, void* stream);
int seg_ssim_backward(const float* img1, const float* img2, int n, int c, int d, int h, int w, int nd, int window, void* ws, const float* gscale,
                      int per_sample, float* dimg1, float* dimg2, void* stream);
/* predict() post-processing on the device (modelVNet.py:670-676): probs [N][C][V] fp32 -> uint8 mask [N][V];
 * C == 1: (p > threshold) * scale (scale 255 or 1); C > 1: first arg-max over the class axis. */
int seg_predict_mask(const float* probs, unsigned char* mask, int n, int c, long long v, float threshold, int scale, void* stream);
/* ---- pre/post-processing either side of predict, planar single-channel volumes [D][H][W].
 * seg_op_resample3d replaces the SimpleITK ResampleImageFilter calls of dataprocess/utils.py:99-145 (identity transform,
 * same origin/direction): output voxel i along an axis samples the input at continuous index i * step, step = output
 * spacing / input spacing (= originSize/newSize for resize_image_itkwithsize, newSpacing/originSpacing for
 * resize_image_itk).  mode 0 = sitkLinear (f32 volumes), 1 = sitkNearestNeighbor (f32 or u8); outside the input
 * buffer (index < -0.5 or >= size - 0.5) the value is 0, as ITK's default pixel.  elem_type 0 = f32, 1 = u8. */
int seg_op_resample3d(const void* src, void* dst, int elem_type, int sd, int sh, int sw, int dd, int dh, int dw,
                      double step_z, double step_y, double step_x, int mode, void* stream);
/* workspace for the two normalisations below (bytes) */
long long seg_op_normalize_ws_bytes(void);
/* ConvertitkTrunctedValue(image, upper, lower, 'meanstd') (dataprocess/utils.py:148-179): optional clip to
 * [lower, upper], then itk::NormalizeImageFilter: (x - mean) / sigma, sigma with the N-1 denominator. */
int seg_op_normalize_meanstd(const float* x, float* out, long long n, int clip, float lower, float upper, void* ws, void* stream);
/* normalize(slice, bottom=95, down=5) (dataprocess/utils.py:182-204): t, b = np.percentile(x, q_lo), np.percentile(x, q_hi)
 * (float32 'linear' method, exact order statistics); x = clip(x, t, b); z-score with the mean / population std of the
 * NON-ZERO clipped voxels; the clipped volume is returned unchanged when either std is 0. */
int seg_op_normalize_percentile(const float* x, float* out, long long n, float q_lo, float q_hi, void* ws, void* stream);
/* inference_patch (model/modelUnet.py:707-763): crop nb windows (origins = nb x {z,y,x} int32, device memory) of
 * pd x ph x pw voxels into a batch [nb][pd][ph][pw]; and the reverse: out[window] = 1 wherever the window's mask is
 * non-zero (out_mask += patch; out_mask[out_mask != 0] = 1).  `out` must be zero-initialised by the caller. */
int seg_op_gather_patches(const float* vol, int d, int h, int w, const int* origins, int nb, int pd, int ph, int pw, float* out, void* stream);
int seg_op_stitch_mask(const unsigned char* masks, const int* origins, int nb, int pd, int ph, int pw, unsigned char* out,
                       int d, int h, int w, void* stream);
/* ---- sliding-window inference with blended probabilities.  A window entry is four int32 {z, y, x, flipbits} in device memory (bit 0
 * mirrors z, bit 1 y, bit 2 x); the same window may be listed several times with different flip bits (mirror augmentation).  Below,
 * (i, j, k) is a position inside a window in volume orientation and a primed index is p - 1 - index on a mirrored axis, index otherwise.
 * seg_op_gather_windows: out[b][i'][j'][k'] = vol[z_b + i][y_b + j][x_b + k], pad_value where that voxel lies outside the volume (a window
 * may overhang, e.g. a volume smaller than the patch along an axis); out is [nb][pd][ph][pw] fp32. */
int seg_op_gather_windows(const float* vol, int d, int h, int w, const int* entries, int nb, int pd, int ph, int pw, float pad_value, float* out,
                          void* stream);
/* For every voxel (z, y, x) of the half-open box box_lo <= (z, y, x) < box_hi (host int[3] each, inside the volume; the caller passes the
 * bounding box of the batch's windows clipped to the volume) and every entry b, in index order, whose window contains the voxel:
 * acc[c][z][y][x] += w * probs[b][c][i'][j'][k'] for c < C and wsum[z][y][x] += w, with (i, j, k) = (z - z_b, y - y_b, x - x_b) and
 * w = (wz[i] * wy[j]) * wx[k] in fp32 (wz / wy / wx: device fp32 importance vectors of pd / ph / pw elements).  probs is [nb][C][pd][ph][pw],
 * acc [C][d][h][w] and wsum [d][h][w] fp32, zeroed by the caller before the first batch; voxels outside the box are not touched.  No
 * atomics: the additions into a voxel happen in entry order, so equal calls give equal bits.  C <= 16. */
int seg_op_blend_windows(const float* probs, const int* entries, int nb, int c, int pd, int ph, int pw, const float* wz, const float* wy,
                         const float* wx, const int* box_lo, const int* box_hi, float* acc, float* wsum, int d, int h, int w, void* stream);
/* acc [C][v], wsum [v] -> mask [v] uint8: C == 1: (acc / wsum > threshold) * scale; C > 1: the first arg-max over acc[c] (the common divisor
 * does not move it).  probs_out (NULL or [C][v] fp32) = acc[c] / wsum.  A voxel with wsum == 0 gives mask 0 and probability 0. */
int seg_op_blend_finalize(const float* acc, const float* wsum, int c, long long v, float threshold, int scale, unsigned char* mask,
                          float* probs_out, void* stream);
/* dice_coeff / iou_coeff / multiclass_* on probabilities (model/metric.py:146-215): out2 = {dice, iou} */
int seg_metric(const float* probs, const void* target, int label_type, int n, int c, long long v,
               void* ws, float* out2, void* stream);

/* torch.optim.AdamW (model/modelVNet.py:548) / Adam (model/modelUnet.py:849) over flat buffers.
 * `state` = int[3] on the device: {step, found_inf, skipped}.  Gradients are multiplied by inv_scale first;
 * with check_finite the update is skipped (state[1] set for this call, state[2] += 1) when any gradient is inf/nan;
 * the caller reads state[2] now and then to back its loss scale off (no per-step host sync). */
int seg_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                  long long numel, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int decoupled, float inv_scale, int check_finite, int* state, void* stream);

/* One whole optimisation step of the reference training loop (model/modelVNet.py:570-596: pred = model(x); loss = lossFunc(pred, y);
 * opt.zero_grad(); loss.backward(); opt.step(), plus the accuracy line :587) enqueued by ONE call:
 * [seg_pack_weights if !packed] -> seg_forward -> seg_loss_forward (out3 = {loss, dice, iou}) -> seg_loss_backward (times the loss
 * scale) -> seg_backward(zero_grads = 1) -> seg_adam_step on the bound params / grads -> seg_pack_weights.  Same launches as the
 * separate calls; the point is one FFI crossing per step.  The rank-local path only: gradient exchange, global-batch losses and the
 * clDice term go through the separate entry points.  grad_div: extra gradient divisor (1 on a single rank). */
typedef struct seg_train_args {
    const float* x; const void* target; int label_type;
    int loss_kind; float focal_alpha, focal_gamma; const float* class_alpha;
    float* logits; float* probs; float* dlogits; void* loss_ws; float* out3;
    int mask_mode; const float* masks; unsigned long long seed;
    float* exp_avg; float* exp_avg_sq; int* opt_state;
    float lr, beta1, beta2, eps, weight_decay; int decoupled; float grad_div; int check_finite;
    int packed;      /* != 0: the run-dtype weight layouts are current (the previous seg_train_step left them so) */
    /* ---- data-parallel exchange hooks (world > 1; all null / 0 for a rank-local step).  The library owns the sequencing of the step, the
     * caller owns the collectives (torch.distributed over RCCL / gloo): each hook is called synchronously from inside seg_train_step at the point
     * of the schedule where its exchange belongs and ENQUEUES the collective (it must not block the host on the device).
     * bucket_cb(user, index, offset, count): the gradient slice grads[offset, offset + count) is final on the device - enqueue its SUM
     *   all-reduce.  The finished slices are suffixes of the flat buffer (gradients finish in reverse registration order); `nfrac` boundaries
     *   `fractions[]` (finished fraction of the buffer, ascending) cut the backward pass into nfrac + 1 buckets (nfrac = 0: one exchange after the
     *   whole backward pass).  With `aux_stream` != null (GPU) the hook for every bucket but the last runs after `aux_stream` has been ordered
     *   behind the caller's stream AND the weight-gradient stream, and is expected to enqueue on `aux_stream`; the caller's stream never waits at
     *   a bucket boundary and meets `aux_stream` again before the last bucket.  Finally bucket_cb(user, -1, 0, 0): order the caller's stream
     *   behind every exchange (the optimiser follows).  Return != 0 aborts the step.
     * loss_cb(user, shared_sums, n_doubles): called between the loss reduction and its finalize with the rank's batch-global fp64 sums (device
     *   pointer): enqueue their SUM all-reduce on the caller's stream; returns the global sample count (0: take it from the exchanged sums,
     *   seg_loss_finalize) or < 0 to abort. */
    int (*bucket_cb)(void* user, int index, long long offset, long long count);
    long long (*loss_cb)(void* user, double* shared_sums, int n_doubles);
    void* cb_user;
    int nfrac; double fractions[4];
    void* aux_stream;
} seg_train_args;
int seg_train_step(seg_handle h, const seg_train_args* a, void* stream);
/* In-library gradient exchange - no host callback between the slices of the backward pass (the hook form above stays as the fallback, and is what
 * the CPU tests with gloo use).  `comm` = an ncclComm_t of RCCL (one rank per GPU; e.g. torch.distributed's: ProcessGroupNCCL._comm_ptr()),
 * `allreduce_fn` = the address of `ncclAllReduce` of the SAME RCCL library that created the communicator:
 *     ncclResult_t (*)(const void* sendbuf, void* recvbuf, size_t count, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t)
 * (the engine does not link RCCL: the caller hands it the function).  While a communicator is set, a seg_train_step with bucket_cb == NULL issues
 * ncclAllReduce(ncclFloat, ncclSum), in place, over every finished suffix of the flat gradient buffer (nfrac / fractions[] as above; nfrac = 0: one
 * all-reduce after the backward pass) on an exchange stream of the library that waits for the caller's stream and the weight-gradient stream (or on
 * a->aux_stream when given); the caller's stream meets it again in front of the optimiser.  a->grad_div carries the 1/world average.  comm == NULL
 * removes the communicator.  A step with a communicator cannot be captured as a HIP graph.  seg_backward_* / seg_adam_step are unaffected. */
int seg_set_rccl_comm(seg_handle h, void* comm, void* allreduce_fn);
/* The same step captured ONCE as a HIP graph (hipStreamBeginCapture around seg_train_step on `stream`, the weight-gradient stream forked and
 * joined inside) and replayed with one hipGraphLaunch per step: for hosts that cannot enqueue ~250 launches per step as fast as the GPU runs
 * them.  Every pointer / scalar of `a` and the current loss scale are baked into the graph (re-capture to change them; seg_plan, seg_bind and
 * seg_set_loss_scale drop the graph); the device-side dropout-draw and Adam step counters keep advancing, so replays are successive steps.
 * a->packed must be 1 (run one ordinary step first).  seg_train_graph_ready: 1 while a captured step exists. */
int seg_train_graph_capture(seg_handle h, const seg_train_args* a, void* stream);
int seg_train_graph_launch(seg_handle h, void* stream);
int seg_train_graph_ready(seg_handle h);

/* ---- operator-level entry points (what torch.nn.functional.conv3d / conv_transpose3d and their
 * autograd weight-gradients are to the reference: networks/VNet3d.py:8,28,29,49,65,70,88).  The
 * network-level calls above are built from exactly these launches; they are exported so each
 * kernel can be checked in isolation.  All tensors channels-last [N][D][H][W][C] in `dtype`. */
typedef struct seg_taps {
    int n;
    signed char d[27], h[27], w[27];
} seg_taps;

/* implicit-GEMM convolution: out[m][co] = sum_{tap,ci} in[vox(m,tap)][ci] * w[co][tap*Cin+ci] (+bias).
 * gather mode (scatter=0): rows m = output voxels (N,OD,OH,OW), input voxel = o*stride + tap.
 * scatter mode (scatter=1): rows m = input voxels, K = Cin, GEMM columns = (tap, co), column block
 * of tap a goes to fine voxel i*up + a (ConvTranspose k2 s2 / data-gradient of conv k2 s2).
 * The reduction input may be a virtual channel concat of in0 (C0 ch) and in1 (C1 ch). */
typedef struct seg_conv_args {
    const void* in0;
    const void* in1;
    int C0, C1;
    const void* w;      /* packed [Ngemm][Kpad] in dtype, zero padded */
    const float* bias;  /* [Cout] or null */
    void* out;
    double* stats;      /* [32][N][Cout][2] sum / sum of squares (+=), 32 replicas to be summed, or null */
    int N, ID, IH, IW;  /* gather source dims */
    int OD, OH, OW;     /* row-space dims */
    int FD, FH, FW;     /* scatter: fine output dims */
    int Cout, Ngemm, K, Kpad;
    int sd, sh, sw;     /* gather: input stride; scatter: up-sampling factor */
    int scatter;
    seg_taps taps;
    /* optional (null: off), gather form on the streaming kernel only (seg_op_conv_kernel == 1): in0 holds the RAW output r of a conv + GroupNorm unit and is read as
     * a = relu(act_scale[n][c] * r + act_shift[n][c]) rounded to dtype - GroupNorm + channel dropout + ReLU of the producer (networks/VNet3d.py:72-74) applied on
     * load, so that the activated tensor is never written; [N][C0] fp32 each */
    const float* act_scale;
    const float* act_shift;
    /* optional (null: off), gather form on the streaming kernel only, no bias / stats: GEMM columns >= Cout0 (a multiple of 16) are written to out1 as rows of
     * Ngemm - Cout0 channels, columns < Cout0 to out as rows of Cout0 channels - the data-gradients of BOTH sources of a virtual concat from one pass over d(raw) */
    void* out1;
    int Cout0;
    /* optional (null: off), with out1 only: `out` (the first Cout0 columns) is the gradient dz of an activation a = relu(rq_scale * r + rq_shift) whose raw tensor
     * r is rq_r ([rows][Cout0] in dtype); the launch adds that unit's GroupNorm-backward sums - sum dz*[a > 0] and sum dz*[a > 0]*r per (sample, channel) - to
     * rq_Q ([32][N][Cout0][2] fp64, replicas to be summed): the reduction pass over (dz, r) that would follow is not needed */
    const void* rq_r;
    const float* rq_scale;
    const float* rq_shift;
    double* rq_Q;
} seg_conv_args;
int seg_op_conv(const seg_conv_args* a, int dtype, void* stream);
/* which kernel seg_op_conv picks for these extents: 1 = register-resident streaming kernel (short reductions on large
 * volumes), 0 = LDS-staged implicit GEMM */
int seg_op_conv_kernel(const seg_conv_args* a);

/* weight gradient dW[p][tap][q] += sum_m dR[m][p] * X[vox(m,tap)][q], written to
 * dw[p*sP + q*sQ + tap*sT] (fp32) through per-slice partial tiles in `partial_scratch`
 * (seg_op_wgrad_partial_bytes bytes; deterministic reduction).  stem=1: X is [N][V][C0] with tiny C0 and q enumerates (tap,ci). */
typedef struct seg_wgrad_args {
    const void* dr;
    const void* x0;
    const void* x1;
    int C0, C1;
    float* dw;
    int P, Q;
    int N, ID, IH, IW, OD, OH, OW;
    int sd, sh, sw;
    seg_taps taps;
    long long sP, sQ, sT;
    int stem;
    /* optional (null: off), 1^d stride-1 convs on 16-bit tensors only (seg_op_wgrad fails otherwise): x0 holds the raw output of a conv + GroupNorm unit and is
     * read as relu(act_scale[n][c] * r + act_shift[n][c]) rounded to dtype, like seg_conv_args.act_scale; [N][C0] fp32 each, C0 <= 64 */
    const float* act_scale;
    const float* act_shift;
} seg_wgrad_args;
long long seg_op_wgrad_partial_bytes(const seg_wgrad_args* a);
int seg_op_wgrad(const seg_wgrad_args* a, float* partial_scratch, int dtype, void* stream);
/* which kernel seg_op_wgrad runs for these arguments now (SEG_WG_S2 is read per call): 0 = wgrad_kernel (voxel gather, one 32-row step in flight),
 * 1 = wgrad_direct_kernel (1^d stride-1 convs on 16-bit tensors), 2 = wgrad_s2_kernel (2^d stride-2 windows on 16-bit tensors, fine extents twice the
 * coarse ones, one source, P a multiple of 32, Q = 16) */
int seg_op_wgrad_kernel(const seg_wgrad_args* a, int dtype);

/* weight re-layout: dst[r1][r2][t][c] (dtype, row length Kpad, zero padded) = src[r1*s1+r2*s2+t'*sT+c*sC],
 * t' = flipT ? T-1-t : t.  `descs` is a DEVICE array. */
typedef struct seg_pack_desc {
    const float* src;
    void* dst;
    int R1, R2, T, Cc;
    int Kpad;
    long long s1, s2, sT, sC;
    int flipT;
    int csrc;   /* channels the SOURCE holds per tap (0: Cc).  csrc < Cc: channels csrc .. Cc-1 of the packed layout are zeros - the image convs of a
                   multi-channel 3-D input, whose image tensor is zero-padded to 16 channels so that they run as ordinary 16-channel halo convs */
    int frag;   /* 0: rows [R1*R2][Kpad]; 1: MFMA-fragment-major [Cc/32][T][rows/16][64 lanes][8] (Cc % 32 == 0, rows % 16 == 0):
                   lane = 16*((c%32)/8) + row%16 holds k = c%8 .. — one 16x32 B fragment is one contiguous 1 KB line;
                   2: the same over the flat k = t*Cc + c axis, [Kpad/32][rows/16][64 lanes][8] (Cc == 16: two taps per step);
                   3: Cc == 16, T == 27, Kpad == 480: [15 steps = kh*5 + pair][rows/16][64 lanes][8], the two taps of a step differ in kd / kw only -
                      pairs 0..2: (kd = pair, kw = 0 | 1), 3: (kd = 0 | 1, kw = 2), 4: (kd = 2, kw = 2 | zeros); read by the tilings whose
                      seg_op_conv3x_cfg_frag(cfg) is 3 */
} seg_pack_desc;
int seg_op_pack(const seg_pack_desc* descs, int ndesc, long long max_elems, int dtype, void* stream);
/* LDS halo-tile kernels for the 3^d (ndim 3) / 3^2 (ndim 2, D = 1) stride-1 pad-1 convolutions.
 * (stats, when given, is [32][N][Cout][2] like seg_conv_args.stats.)
 * seg_op_conv3: out[N][D][H][W][Cout] = conv(in[N][D][H][W][Cin], w packed [Cout][Kpad], k = (tap, ci)) + bias,
 * optional GroupNorm partial sums; with the "conv_dgrad" weight layout it is the data-gradient.
 * seg_op_wgrad3: dw[p][q][tap] += sum_m dr[m][p] * x[m + tap][q]; `partial` needs
 * seg_op_wgrad3_partial_bytes(...) bytes of scratch (deterministic two-stage reduction). */
int seg_op_conv3(const void* in, const void* w, const float* bias, void* out, double* stats, int n, int d, int h,
                 int wid, int cin, int cout, int ndim, int dtype, void* stream);
long long seg_op_wgrad3_partial_bytes(int ndim, int n, int d, int h, int wid, int p, int q);
int seg_op_wgrad3(const void* dr, const void* x, float* partial, float* dw, int n, int d, int h, int wid, int p,
                  int q, int ndim, int dtype, void* stream);
/* seg_op_wgrad3 with x a virtual channel concat: channels [0, c0) of x come from x0 ([..][c0]), the rest from x1 ([..][q - c0])
 * (the UNet decoder blocks read cat(up, skip), networks/Unet3d.py:50-62, without materialising it). */
int seg_op_wgrad3_cat(const void* dr, const void* x0, const void* x1, int c0, float* partial, float* dw, int n, int d, int h,
                      int wid, int p, int q, int ndim, int dtype, void* stream);
/* Fused input block (csrc/stemx.hip): y = relu(drop(GN(conv3(x)))) [+ relu(drop(GN(conv1(x))))] for a 1..3-channel image and 16
 * output channels (InputTransition of networks/VNet3d.py:25-43 with its shared GroupNorm module applied twice; first conv of
 * networks/Unet3d.py:64-86 with w1 = NULL).  The raw conv outputs are recomputed in every pass instead of being stored.
 * mode 0: GroupNorm partial sums of both branches -> stats3 / stats1 ([32][N][16][2] fp64, accumulated);
 * mode 1: out[N][D][H][W][16] from scale / shift ([N][16], dropout multiplier folded in);
 * mode 2: Q3 / Q1 ([32][N][16][2]: sum dz, sum dz*r with dz = (sum of the ndy gradient sources) * [scale*r + shift > 0]);
 * mode 3: weight gradients: d(raw) = coef[0]*dz + coef[1]*r + coef[2] (coef [N][16][3]) times the im2col rows, accumulated
 *         into dw3 (16, Cimg, 3^d) / dw1 (16, Cimg, 1^d) through `partial` (seg_op_stemx_partial_bytes of scratch).
 * mode 4: mode 2's Q3 / Q1 plus, in the same pass, the per-workgroup moments of the weight gradients in `partial` (seg_op_stemx_moment_bytes of
 *         scratch; a workgroup stays inside one sample): T1 = sum patch*dz, T2 = sum patch*r, T3 = sum patch over the valid voxels (fp32);
 * mode 5: the combine: dw3 / dw1 += sum_n coef[n][co][0]*T1 + coef[n][co][1]*T2 + coef[n][co][2]*T3 from mode 4's `partial`, folded in fp64 in a fixed
 *         order (takes coef3 / coef1, partial, the shape and w1 != NULL for two branches; modes 4 + 5 replace modes 2 + 3 - dz instead of d(raw) is
 *         rounded to the run dtype, so the two are equal up to rounding, and exactly equal on data whose products and sums are exact).
 * w3 / w1: run-dtype [16][32] rows, k = tap*Cimg + ci / k = ci (seg_op_pack "conv_fwd" layout).  img: run dtype, channels-last. */
typedef struct seg_stemx_args {
    const void* img; const void* w3; const void* w1;
    const float* bias3; const float* bias1;
    double* stats3; double* stats1;
    const float* scale3; const float* shift3; const float* scale1; const float* shift1;
    void* out;
    const void* dy[3]; int ndy;
    double* Q3; double* Q1;
    const float* coef3; const float* coef1;
    float* partial;
    int N, D, H, W, Cimg;
} seg_stemx_args;
long long seg_op_stemx_partial_bytes(int ndim, int n, int d, int h, int wid, int cimg);
long long seg_op_stemx_moment_bytes(int ndim, int n, int d, int h, int wid, int cimg);
int seg_op_stemx(const seg_stemx_args* a, int mode, int ndim, int dtype, float* dw3, float* dw1, void* stream);
/* Register-blocked halo conv for 16-bit tensors with Cin % 32 == 0 or Cin == 16 (csrc/conv3x.hip): same operator as seg_op_conv3, the
 * weights packed with seg_pack_desc.frag = seg_op_conv3x_cfg_frag(cfg) (1; Cin == 16: 2 or 3) ("conv_fwd" / "conv_dgrad" element order), `in1` an optional second source of a
 * virtual channel concat (channels c0..cin-1).  cfg selects a tiling (seg_op_conv3x_cfg_info enumerates them; -1 = the
 * engine's default for the shape).  Returns <0 when the tiling does not fit the shape. */
int seg_op_conv3x(int cfg, const void* in0, const void* in1, int c0, const void* w, const float* bias, void* out, double* stats,
                  int n, int d, int h, int wid, int cin, int cout, int ndim, int dtype, void* stream);
int seg_op_conv3x_num_cfgs(void);
/* index in [0, num_cfgs): tiling id, ndim, box {d,h,w}, output channels per workgroup, resident 32-channel chunks, description */
int seg_op_conv3x_cfg_info(int index, int* id, int* ndim, int* box3, int* bn, int* nres, char* name, int name_cap);
int seg_op_conv3x_default_cfg(int ndim, int n, int d, int h, int wid, int cin, int cout, int dtype);
/* seg_pack_desc.frag of the weights tiling `cfg` reads: 1, 2 (Cin == 16) or 3 (Cin == 16, 3-D, the halo fragments reused across the kh taps:
 * csrc/conv3x_impl.h conv3x16r_kernel); 0 for an unknown id.  This call, not an id range, says which layout a tiling reads (today 3 for tilings 28 and 29) */
int seg_op_conv3x_cfg_frag(int cfg);
/* sizeof of the structs of this header as compiled into the library: 0 conv, 1 wgrad, 2 pack, 3 stemx, 4 train, 5 gn_fwd, 6 gn_bwd */
int seg_abi_sizeof(int which);

/* ---- GroupNorm(8) + channel dropout + ReLU (+ second branch, + residual) and max-pool, one operator at a time (csrc/norm.hip, csrc/misc.hip):
 * the launches the engine issues, with the path named by the caller.  A path whose own eligibility rule says no is an error and nothing is launched.
 * Tensors [N][V][C] in the run dtype, C in {16, 32, 64, 128, 256}; statistics `stats` [32][N][C][2] fp64 = per-channel {sum r, sum r^2}, spread over the
 * first `rep` (1..32) replicas, the other replicas zero; gamma / beta [C]; mask [N][mask_ld] dropout multipliers or null.
 *   out = relu(scale1 * r1 + shift1) [+ relu(scale2 * r2 + shift2)] [+ res],  scale = mask * gamma * rstd,  shift = mask * (beta - gamma * mean * rstd)
 * scale / shift [N][C] and mean / rstd [N][8] are outputs.  The second branch (r2 != null) has its own statistics, parameters and outputs. */
enum { SEG_GN_FWD_FINALIZE = 0,   /* gn_finalize launch, then the elementwise pass */
       SEG_GN_FWD_FOLD = 1,       /* the elementwise pass folds the statistics itself */
       SEG_GN_FWD_GROUP = 2 };    /* one workgroup per (sample, group): seg_op_gn_group_eligible, no second branch */
typedef struct seg_gn_fwd_args {
    const void* r1; const void* r2; const void* res; void* out;
    const double* stats1; const double* stats2;
    const float* gamma1; const float* beta1; const float* gamma2; const float* beta2;
    const float* mask1; const float* mask2; int mask_ld;
    float* scale1; float* shift1; float* mean1; float* rstd1;
    float* scale2; float* shift2; float* mean2; float* rstd2;
    int N, C; long long V;
    float eps; int rep; int path;
} seg_gn_fwd_args;
int seg_op_gn_forward(const seg_gn_fwd_args* a, int dtype, void* stream);
/* The backward of the same unit.  Gradient sources: ndy (0..3) stored tensors dy[i] plus the optional virtual head source
 * dy[n][v][c] += sum_k vdl[n][k][v] * vw[k][c] (vdl planar fp32 [N][vK][V], vw [vK][C]); dz = (their sum) * [scale * r + shift > 0].
 * scale / shift / mean / rstd / stats / gamma / mask: as the forward left them (inputs).  Q [32][N][C][2] fp64 must be ZERO at the call:
 * the reduce launch leaves {sum dz, sum dz * r} spread over its first rep_q replicas, the co-operative kernel uses it as its exchange area
 * ([N][8][S][C/8] words of two floats).  coef [N][C][3] = (A, B, Cc) (written by the first two paths), dr = A * dz + B * r + Cc;
 * dgamma / dbeta / dbias [C] fp32 are accumulated into (dbias may be null).  A second branch (r2 != null: its own scale2 .. dr2, fed by the same
 * gradient sources) exists on the first two paths only. */
enum { SEG_GN_BWD_SEPARATE = 0,   /* reduce, finalize, apply: three launches */
       SEG_GN_BWD_FOLD = 1,       /* reduce, then an apply launch that folds the finalize */
       SEG_GN_BWD_GROUP = 2,      /* one workgroup per (sample, group): seg_op_gn_group_eligible, stored sources only */
       SEG_GN_BWD_COOP = 3 };     /* S workgroups per (sample, group): seg_op_gn_coop_plan, 1..3 stored sources only */
typedef struct seg_gn_bwd_args {
    const void* dy[3]; int ndy;
    const float* vdl; const float* vw; int vK;
    const void* r; const void* r2;
    const float* scale; const float* shift; const float* scale2; const float* shift2;
    const float* mean; const float* rstd; const float* mean2; const float* rstd2;
    const double* stats; const double* stats2;
    const float* gamma; const float* gamma2;
    const float* mask; const float* mask2; int mask_ld;
    double* Q; double* Q2;
    float* coef; float* coef2;
    void* dr; void* dr2;
    float* dgamma; float* dbeta; float* dbias;
    float* dgamma2; float* dbeta2; float* dbias2;
    int N, C; long long V;
    int rep_q, rep_s; int path;
} seg_gn_bwd_args;
int seg_op_gn_backward(const seg_gn_bwd_args* a, int dtype, void* stream);
/* The same (SEPARATE / FOLD paths, one branch, the virtual source of a one-class head: vK == 1, ndy 0 or 1, C <= 128), and the reduce launch also collects
 * the head's weight gradient: head_dw[c] += sum_{n,v} vdl[n][v] * act[n][v][c], act = relu(scale * r + shift) - in fp32 for ndy == 0, which also gives
 * head_db[0] += sum vdl; rounded to the run dtype (the activation as a forward pass stores it) for ndy == 1, head_db untouched.  head_sums: scratch
 * shaped like Q, ZERO at the call. */
int seg_op_gn_backward_head(const seg_gn_bwd_args* a, double* head_sums, float* head_dw, float* head_db, int dtype, void* stream);
/* the co-operative kernel's plan for a shape (esz: bytes per element): 1 and *S workgroups per (sample, group), *ku chunks per thread; 0: not eligible */
int seg_op_gn_coop_plan(int c, long long v, int n, int esz, int* S, int* ku);
int seg_op_gn_group_eligible(int c, long long v, int esz);
/* max-pool with window = stride = (pd, ph, pw), each 1 or 2 and a divisor of its extent, on [N][D][H][W][C] (C % 8 == 0).  backward = 0: out = pool(in);
 * backward = 1: din (fine) = dout (coarse) routed to the first maximum of each window of `in` in (d, h, w) scan order, zero elsewhere. */
int seg_op_maxpool(const void* in, void* out, const void* dout, void* din, int n, int d, int h, int w, int c, int pd, int ph, int pw,
                   int backward, int dtype, void* stream);
/* Classification head of SEG_NET_RESNET (networks/ResNet3d.py:61-69,91-96,114-116) on the channels-last activation act [N][V][256] (run dtype):
 *   pooled[n][k] = mean_v act[n][v][k]        h = relu(W1 pooled + b1), W1 [128][256]        logits = W2 h + b2, W2 [C][128]        probs = sigmoid (C == 1) / soft-max
 * forward leaves pooled (N x 256) and h (N x 128), fp32, in `ws` (seg_op_cls_head_ws_bytes(n, v) bytes, 256-byte aligned) for the backward call, which
 * takes dlogits [N][C] (times the loss scale) and gives dW2 = dl^T h, db2, dh = (W2^T dl) [h > 0], dW1 = dh^T pooled, db1 and
 * dact[n][v][k] = (W1^T dh)[n][k] / V in the run dtype.  zero_grads = 0: the parameter gradients are ADDED to what the four buffers hold; 1: they replace it.
 * Nothing is read back, no grid depends on data and there are no floating-point atomics: the voxel sum is an fp64 sum per 64-voxel slab (ascending voxels)
 * folded over the slabs in ascending order, the FC dot products are fp32 fmaf chains in a fixed lane order, every sum over samples runs over ascending n -
 * two calls agree bit for bit.  n >= 1, 1 <= v < 2^31 / 256, 1 <= c <= 16.  seg_op_cls_head_ws_offset: the byte offset of pooled / h inside `ws`. */
long long seg_op_cls_head_ws_bytes(int n, long long v);
long long seg_op_cls_head_ws_offset(int n, long long v, int what /* 0: pooled, 1: h */);
int seg_op_cls_head_forward(const void* act, const float* w1, const float* b1, const float* w2, const float* b2, float* logits, float* probs, int n,
                            long long v, int c, void* ws, int dtype, void* stream);
int seg_op_cls_head_backward(const float* dlogits, const float* w1, const float* w2, float* dw1, float* db1, float* dw2, float* db2, void* dact, int n,
                             long long v, int c, int zero_grads, void* ws, int dtype, void* stream);
/* Grad-CAM of one layer (csrc/gradcam.hip; model/visualization.py:135-193 of the reference) on act / grad [N][ID][IH][IW][C] in the run dtype, C in
 * {16, 32, 64, 128, 256}, grad = (gradient of the class score) / inv_loss_scale.  Per sample n:
 *   w[c] = inv_loss_scale * mean_v grad[n][v][c]          fp64 sums per 512-voxel slab, folded over ascending slabs, rounded once to fp32
 *   cam[v] = max(0, sum_c w[c] act[n][v][c])               fp32 fmaf chain
 *   s = (cam - min cam) / (1e-7 + (max cam - min cam))     min / max over the sample (a constant cam, one voxel included, gives s = 0)
 *   r = s resized to (OD, OH, OW): linear along every axis, source coordinate (o + 0.5) * in / out - 0.5 clamped to the axis - cv2 INTER_LINEAR as
 *       published (cv2.resize itself is not pinned: the reference needs it, this project's tests do not have it), which equals
 *       F.interpolate(mode = "bilinear" / "trilinear", align_corners = False) when enlarging
 *   out[n] = weight * r (accumulate = 0)  or  out[n] + weight * r (accumulate != 0)
 *   finalize != 0: then out[n] = (q - min q) / (1e-7 + (max q - min q)), q = max(0, out[n])   (aggregate_multi_layers)
 * so a map over L layers is L calls with weight = 1 / L, accumulate = 0 for the first, finalize = 1 for the last.  ndim 2: ID = OD = 1.  act / grad
 * 32-byte aligned; ws: seg_op_gradcam_ws_bytes() bytes, 256-byte aligned.  n 1..65535, id * ih * iw * c and od * oh * ow below 2^31.  Stream-ordered, no
 * allocation, no readback, no floating-point atomics: two calls agree bit for bit. */
long long seg_op_gradcam_ws_bytes(int n, int c, int id, int ih, int iw, int od, int oh, int ow);
int seg_op_gradcam(const void* act, const void* grad, int dtype, int n, int c, int id, int ih, int iw, int od, int oh, int ow, int ndim, float inv_loss_scale,
                   float weight, int accumulate, int finalize, void* ws, float* out, void* stream);

/* ---- soft-clDice building blocks (model/lossescldice.py:5-59; corrected restatement).
 * Planar fp32 tensors [planes][D][H][W]; nd = 3 pools 3x3x3 over (D,H,W), nd = 2 pools 3x3 over (H,W); stride 1, pad 1,
 * padding ignored.  seg_op_skel_update: out = relu(x - relu(maxpool(e) - e)).  The *_bwd entry points route gradients to the
 * first extremum of each window (ATen max_pool backward); `de` / `din` are accumulated into (zero them first). */
int seg_op_pool3(const float* x, float* out, int planes, int d, int h, int w, int nd, int is_min, void* stream);
/* one whole skeleton iteration (e_out = minpool(x), x_out = relu(x - relu(maxpool(e_out) - e_out))) in one pass over LDS tiles;
 * bit-identical to seg_op_pool3(is_min) + seg_op_skel_update */
int seg_op_skel_iter(const float* x, float* e_out, float* x_out, int planes, int d, int h, int w, int nd, void* stream);
/* backward of seg_op_skel_iter: dx = d loss / d x given g = d loss / d x_out (x, e as saved by the forward); two gather passes
 * over LDS tiles - deterministic, no atomics; `de_scratch` is a tensor-sized fp32 work buffer (need not be cleared) */
int seg_op_skel_iter_bwd(const float* g, const float* x, const float* e, float* dx, float* de_scratch, int planes, int d, int h, int w,
                         int nd, void* stream);
int seg_op_skel_update(const float* x, const float* e, float* out, int planes, int d, int h, int w, int nd, void* stream);
int seg_op_skel_update_bwd(const float* g, const float* x, const float* e, float* dx, float* de, int planes, int d, int h, int w,
                           int nd, void* stream);
int seg_op_pool3_bwd(const float* src, const float* dout, float* din, int planes, int d, int h, int w, int nd, int is_min,
                     void* stream);
/* out2[p] = {sum a*b, sum a} per plane (fp64; `scratch` = seg_op_plane_dot_scratch_bytes bytes of per-workgroup partials);
 * out = a[p]*in + b[p] (accumulate != 0: +=) */
long long seg_op_plane_dot_scratch_bytes(int planes, long long v);
int seg_op_plane_dot(const float* a, const float* b, double* out2, double* scratch, int planes, long long v, void* stream);
int seg_op_plane_axpb(const float* in, const float* a, const float* b, float* out, int planes, long long v, int accumulate,
                      void* stream);

/* Binary soft-clDice as a loss of the engine (reference: model/lossescldice.py:37-59 Binary_Soft_cldice_loss, with the repairs listed in
 * oracle/make_golden.py:CLDICE_REPAIRS; `width` = skeleton iterations, 10 in the reference).  probs = the head's probabilities
 * [n][1][d][h][w] fp32, target = labels of the same extent.  out1[0] = the clDice loss; when dlogits != NULL,
 * grad_scale * d loss / d logit (sigmoid Jacobian included) is ADDED to dlogits, i.e. call it after seg_loss_backward of the
 * companion loss (Dice) with grad_scale = weight * loss scale.  ws: seg_cldice_ws_bytes() bytes planned by the caller; no
 * allocation, no host synchronisation.  nd = 2 (d = 1) or 3.
 * The target is ALWAYS read as the binary mask (label != 0), whatever `label_type` says (SEG_LABEL_BINARIZE is implied): that is what the
 * reference's train loop hands to every loss (model/modelVNet.py:576 binarises the labels first), and it lets the target's skeleton be computed on a
 * bit image.  A caller with soft (fractional) targets - which Binary_Soft_cldice_loss.forward itself would skeletonise as given - must use the
 * building blocks above (seg_op_skel_iter, seg_op_plane_dot, ...); the companion loss keeps reading the labels as `label_type` says. */
long long seg_cldice_ws_bytes(int n, int d, int h, int w, int nd, int width);
/* optional: the label-only part (float labels + the target skeleton) into ws ahead of time, e.g. on another stream while the forward pass
 * runs; seg_cldice_binary(target_ready = 1) then skips it (the caller orders the two calls with an event). */
int seg_cldice_target(const void* target, int label_type, int n, int d, int h, int w, int nd, int width, void* ws, void* stream);
int seg_cldice_binary(const float* probs, const void* target, int label_type, int n, int d, int h, int w, int nd, int width,
                      float grad_scale, void* ws, float* out1, float* dlogits, int target_ready, void* stream);

/* ---- Seg_Metirc3d (model/metric.py:11-142) on the device: the four overlap counts and the symmetric surface distances of two label volumes
 * [d][h][w] (uint8) in one call (csrc/surface.hip).  A voxel belongs to the mask when label == cls, or when label != 0 for cls == -1 (the
 * reference's binary case).  Surface = mask voxels with one of their 18 neighbours outside the mask or outside the volume (binary_erosion with
 * generate_binary_structure(3, 2), border_value 0); nearest distances by an exact all-pairs search with the spacing (sz, sy, sx) of the (d, h, w) axes
 * rounded to f32.  out16 (device memory, 16 doubles) = {|R|, |P|, |R n P|, |R u P|, n_surf_R, n_surf_P, sum r2p, sum p2r, sum r2p^2, sum p2r^2,
 * max r2p, max p2r, 0, 0, 0, 0}; with an empty surface on either side the six counts are still correct and the six distance fields are NaN.
 * real2pred_nn / pred2real_nn: NULL, or room for d*h*w floats each; they receive the per-point distances in raster order of the surface points.
 * ws: seg_surface_ws_bytes() bytes, 256-byte aligned, sized for the case that every voxel is a surface voxel (a checkerboard): 16.3 bytes per voxel
 * (four uint32 per voxel, two ballot bits per voxel, 32 bytes per 4096 voxels) + 13 KB.  After the call ws holds the packed linear indices
 * ((z*h + y)*w + x, uint32, raster order) of the real surface at byte 0 and of the pred surface at byte 256*ceil(4*d*h*w / 256).
 * Limits: 1 <= d, h, w <= 2048 and d*h*w < 2^31 (with unit spacing every squared distance is then an integer f32 holds exactly).
 * No allocation, no host synchronisation, no grid that depends on a count; two calls on the same input agree bit for bit. */
long long seg_surface_ws_bytes(int d, int h, int w);
int seg_surface_metrics(const unsigned char* real, const unsigned char* pred, int d, int h, int w, int cls,
                        double sz, double sy, double sx, void* ws, double* out16,
                        float* real2pred_nn, float* pred2real_nn, void* stream);

/* ---- ImageDataGenerator3D (dataprocess/Augmentation/images_masks_3dtransform.py:63-269) on the device: a batch of images and their label volumes
 * through per-sample affine transforms in ONE launch (csrc/augment.hip) - scipy.ndimage.affine_transform(order = 0) per channel in the reference.
 * x / out: f32, n samples of c channels on the grid (n0, n1, n2); element (s, ch, i0, i1, i2) lives at s*c*V + ch*xs_c + ((i0*n1 + i1)*n2 + i2)*xs_v with
 * V = n0*n1*n2, so (N, C, D, H, W) is (xs_c, xs_v) = (V, 1) and the reference's channel-last (N, n0, n1, n2, C) is (1, c).  out != x, same layout.
 * label / label_out: NULL, or SEG_LABEL_U8 / _I64 / _F32 volumes on the same grid with label_c channels: 1 (no channel axis), or c (the image's strides).
 * params_dev: device memory, SEG_AUGMENT_PARAM_DOUBLES doubles per sample: [0..8] the 3x3 matrix A row-major, [9..11] the offset, [12] the flips
 * (1: axis 0, 2: axis 1, 4: axis 2, or-ed), [16 + ch] the channel shift u_ch (read by seg_augment3d_shift, ch < 8), the rest 0.  params_host: the same block
 * in host memory; it is only validated (finite matrix and offset, flips 0..7) and need not outlive the call - uploading it is the caller's business.
 * Output voxel o = (i0, i1, i2) takes the input voxel at floor(cc_a + 0.5) per axis a, cc_a = ((i0*A[a][0] + i1*A[a][1]) + i2*A[a][2]) + off[a] in double
 * without fused multiply-add; SEG_AUGMENT_NEAREST clamps cc_a to [0, n_a - 1], SEG_AUGMENT_CONSTANT gives cval (label: label_cval) to a voxel with any
 * cc_a < 0 or cc_a > n_a - 1.  The value is stored at the flipped position of o.  rescale != 0: out = v * (float)rescale (image only).  extrema != 0:
 * instead of rescaling, the minimum and maximum of every transformed sample (all channels) are left in ws for seg_augment3d_shift.
 * seg_augment3d_shift (in place, same layout arguments): x = clip(x + (float)u_ch, min, max) when params_dev != NULL (needs c <= 8 and the ws of a
 * seg_augment3d call with extrema != 0 on the same stream), then x *= (float)rescale when rescale != 0.
 * ws: seg_augment3d_ws_bytes(n) bytes (256 per sample), 256-byte aligned.  Errors (nothing is launched): null pointers, n outside 1..65535, an extent
 * below 1 or n0*n1*n2 above 2^31, a non-finite matrix / offset / cval, SEG_AUGMENT_REFLECT / _WRAP (not implemented), a label_cval an integer label type
 * cannot hold (mode constant).  Stream-ordered, no allocation, no readback, no synchronisation; no parameter value can make a read leave the input. */
enum { SEG_AUGMENT_NEAREST = 0, SEG_AUGMENT_CONSTANT = 1, SEG_AUGMENT_REFLECT = 2, SEG_AUGMENT_WRAP = 3, SEG_AUGMENT_PARAM_DOUBLES = 24 };
long long seg_augment3d_ws_bytes(int n);
int seg_augment3d(const float* x, float* out, int n, int c, int n0, int n1, int n2, long long xs_c, long long xs_v,
                  const void* label, void* label_out, int label_type, int label_c, const double* params_host, const double* params_dev,
                  int fill_mode, double cval, double label_cval, double rescale, int extrema, void* ws, void* stream);
int seg_augment3d_shift(float* x, int n, int c, int n0, int n1, int n2, long long xs_c, long long xs_v, const double* params_dev,
                        double rescale, const void* ws, void* stream);

/* ---- Segmenation_Aug (dataprocess/AugData.py of the reference: an albumentations Compose) on the device: a batch of 2-D images and their label images
 * through per-sample flips, one blur, an affine warp and brightness / contrast in ONE launch (csrc/augment2d.hip).  The arithmetic below IS the contract:
 * it is not pinned to albumentations / cv2 (neither can run where this library is built and tested, and their draw order and uint8 fixed-point
 * interpolation differ between their own versions); tests/aug2d_oracle.py restates it in float64.
 * x / out: f32, n samples of c channels on the grid (h, w); element (s, ch, y, x) of the input lives at s*xs_n + ch*xs_c + (y*w + x)*xs_v, of the output
 * at s*c*V + ch*xs_c + (y*w + x)*xs_v with V = h*w: (N, C, H, W) is (xs_n, xs_c, xs_v) = (c*V, V, 1), channel-last (N, H, W, C) is (c*V, 1, c).
 * xs_n == 0: all n outputs are variants of ONE source image (and one source label); otherwise xs_n >= c*V.  out != x.
 * label / label_out: NULL, or SEG_LABEL_U8 / _I64 / _F32 images [n][h][w] (one channel).
 * params_dev: device memory, SEG_AUGMENT2D_PARAM_DOUBLES doubles per sample; params_host: the same block in host memory, only validated:
 *   [0..5] M row-major 2x3   [6] flips (1 horizontal, 2 vertical, or-ed)   [7] warp   [8] blur   [9] k   [10] alpha   [11] beta   [12] clip
 *   [13] clip_lo   [14] clip_hi   [15] 0 - or weight 48, the last of a 7 x 7 kernel, which 16 + 49 slots would need one more double for
 *   [16..64) the k*k blur weights row-major (the first 48 of a 7 x 7 kernel), the rest 0
 * Output pixel (y, x) of a sample, every channel alike:
 *   1. flip   F(y, x) = src(vflip ? h-1-y : y, hflip ? w-1-x : x)
 *   2. blur   (image only)  0: G = F.  1: G = correlation of F with the k x k weights (k 3, 5 or 7, anchor at the centre, weights and sum in f32; a tap
 *             outside the image reads index i folded with period 2(n-1), 0 for n == 1: d c b | a b c d, cv2's BORDER_REFLECT_101).
 *             2: the 3 x 3 median with replicated edges - a selection, no arithmetic.
 *   3. warp   skipped when warp == 0 (G passes bit for bit).  sy = (y*M[0][0] + x*M[0][1]) + M[0][2], sx from row 1, in double without fused
 *             multiply-add.  Image: bilinear over floor(sy), floor(sy)+1 and floor(sx), floor(sx)+1 with f32 weights
 *             (1-wy)*((1-wx)*g00 + wx*g01) + wy*((1-wx)*g10 + wx*g11); the blur is evaluated at the taps.  Label: the pixel at floor(sy + 0.5),
 *             floor(sx + 0.5).  border_mode: SEG_AUGMENT_MIRROR folds an index as the blur does, however far out; SEG_AUGMENT_NEAREST clamps it;
 *             SEG_AUGMENT_CONSTANT gives cval to a tap outside and label_cval to a label pixel outside.  _REFLECT and _WRAP are refused.
 *   4. tone   (image only)  v = alpha*v + beta in f32 unless alpha == 1 and beta == 0; then clamp to [clip_lo, clip_hi] when clip != 0.
 * With blur 0 or 2, warp 0, alpha 1, beta 0 and clip 0 every output value is a bit copy of an input value.
 * ws: seg_augment2d_ws_bytes(n) bytes - 0 today, ws may then be NULL.  Errors (nothing is launched): a null pointer, n outside 1..65535, an extent
 * below 1 or h*w above 2^31, strides that leave a sample, non-finite M / alpha / beta / cval / weights, blur outside 0..2, k outside {3, 5, 7} when
 * blur == 1, flips outside 0..3, clip_lo > clip_hi, a refused or unknown border mode, a label_cval an integer label type cannot hold (mode constant),
 * out == x.  Stream-ordered, no allocation, no readback, no synchronisation; no parameter value can make a read leave the input. */
enum { SEG_AUGMENT_MIRROR = 4, SEG_AUGMENT2D_PARAM_DOUBLES = 64 };
long long seg_augment2d_ws_bytes(int n);      /* may return 0 */
int seg_augment2d(const float* x, float* out, int n, int c, int h, int w, long long xs_n, long long xs_c, long long xs_v,
                  const void* label, void* label_out, int label_type, const double* params_host, const double* params_dev,
                  int border_mode, double cval, double label_cval, void* ws, void* stream);

/* ---- mask post-processing (dataprocess/utils.py:7-96 of the reference) on the device (csrc/postproc.hip): connected components and binary morphology
 * of n independent uint8 volumes [n][d][h][w] (2-D: d = 1).  A voxel is foreground when value == cls, or when value != 0 for cls == -1.  Nothing
 * connects or spreads across samples.  Limits: 1 <= d, h, w <= 2048, 1 <= n <= 65535, n*d*h*w < 2^31.
 *
 * seg_cc_label.  connectivity 1: faces (6 neighbours, 4 for d = 1; ITK's ConnectedComponent and scipy.ndimage.label default); 3: fully connected (26 / 8).
 * labels: NULL, or n*d*h*w int32: 0 for background, components numbered 1..K per sample in raster order (x fastest) of each component's first voxel -
 * scipy.ndimage.label's numbering.  stats: device memory, SEG_CC_STATS_INTS int32 per sample:
 *   [0] K   [1] foreground voxels   [2] size of the largest component   [3] its label number   [4] in-sample linear index (z*h + y)*w + x of its first voxel
 *   [5..10] inclusive bounding box z0 y0 x0 z1 y1 x1 of the largest component   [11..16] the same of the whole foreground   [17..31] 0
 * An empty foreground gives K 0, size 0, label 0, index -1 and boxes {d, h, w, -1, -1, -1}.  Of several largest components the one whose first voxel
 * comes first in raster order is taken (a loop with `maxsize < size` over ascending labels keeps the same one).
 * seg_cc_filter.  SEG_CC_KEEP_LARGEST: out = the input value where the voxel belongs to the largest component, else 0; SEG_CC_MIN_SIZE: the same for every
 * component of at least min_voxels voxels.  out may be mask; stats may be NULL.  The decision is taken on the device, nothing is read back.
 * ws: seg_cc_ws_bytes() bytes, 256-byte aligned: 12 bytes per voxel (parent, root and size per voxel slot) + 20 bytes per 64-voxel row word + 160 per sample.
 *
 * seg_morph3d.  out = fg_value where the result is set, else 0; out may be mask.  op: SEG_MORPH_*; shape with per-axis radii 0..31: SEG_SE_BOX the full
 * (2r+1) cuboid, SEG_SE_CROSS the three axis segments, SEG_SE_BALL the offsets with sum_a (delta_a / (r_a + 0.5))^2 <= 1 over the axes with r_a > 0 and
 * delta_a = 0 on the others (ITK's FlatStructuringElement::Ball with a non-parametric radius as published: 19 voxels for (1,1,1), 81 for (2,2,2), 179 for
 * (3,3,3), 9 for (0,1,1)).  border: the value assumed outside the volume, 0 or 1; -1 = 0 for a dilation, 1 for an erosion.  SEG_MORPH_OPEN =
 * dilate(erode(x, 1), 0), SEG_MORPH_CLOSE = erode(dilate(x, 0), 1); they take border -1 only.  Equal to scipy.ndimage.binary_dilation / binary_erosion
 * with structure = the element and border_value = border.  ws: seg_morph3d_ws_bytes() bytes (two bit planes), 256-byte aligned.
 *
 * All calls: stream-ordered, no allocation, no host synchronisation, no grid that depends on the data, integer arithmetic only - two calls on the same
 * input agree bit for bit.  Errors (nothing is launched, seg_last_error() says which): null pointers, limits, a connectivity other than 1 or 3, unknown
 * mode / op / shape, a radius outside 0..31, an explicit border with open / close, fg_value outside 0..255. */
enum { SEG_CC_STATS_INTS = 32, SEG_CC_KEEP_LARGEST = 0, SEG_CC_MIN_SIZE = 1 };
enum { SEG_MORPH_DILATE = 0, SEG_MORPH_ERODE = 1, SEG_MORPH_OPEN = 2, SEG_MORPH_CLOSE = 3, SEG_SE_BALL = 0, SEG_SE_BOX = 1, SEG_SE_CROSS = 2 };
long long seg_cc_ws_bytes(int n, int d, int h, int w);
int seg_cc_label(const unsigned char* mask, int n, int d, int h, int w, int cls, int connectivity, void* ws, int* labels, int* stats, void* stream);
int seg_cc_filter(const unsigned char* mask, unsigned char* out, int n, int d, int h, int w, int cls, int connectivity, int mode,
                  long long min_voxels, void* ws, int* stats, void* stream);
long long seg_morph3d_ws_bytes(int n, int d, int h, int w);
int seg_morph3d(const unsigned char* mask, unsigned char* out, int n, int d, int h, int w, int cls, int op, int shape, int rz, int ry, int rx,
                int border, int fg_value, void* ws, void* stream);

/* ---- exact Euclidean distance transform (csrc/edt.hip) of n independent uint8 volumes [n][d][h][w] (2-D: d = 1), and the boundary loss that consumes
 * its maps (Kervadec et al., "Boundary loss for highly unbalanced segmentation").  A voxel is foreground when label == cls, or when label != 0 for
 * cls == -1 (seg_cc_label's convention).
 *
 * seg_edt.  For every foreground voxel the Euclidean distance to the nearest background voxel OF THE SAME SAMPLE, with the spacing (sz, sy, sx) of the
 * (d, h, w) axes; background voxels get 0; nothing outside the volume counts as background (scipy.ndimage.distance_transform_edt's convention, not the
 * morphology's border).  The transform is exact, separable and linear in the voxel count: axis x from the bit-packed rows, axes y and z as lower
 * envelopes of parabolas; no radius, no approximation.  Squared distances come from integer index differences.  With unit spacing the whole computation
 * is integer (d^2 <= 3 * 2047^2 < 2^24): the f32 stored is the exact integer and the root is correctly rounded.  Otherwise the spacings are rounded to
 * f32 once, d^2 = sum_a (delta_a * s_a)^2 in f32, and the minimum is taken over true candidates.
 * mode: SEG_EDT_SQUARED / SEG_EDT_DISTANCE  d^2 / d on the foreground, 0 on the background;
 *       SEG_EDT_SIGNED    + distance to the foreground outside the mask, - distance to the background inside (two transforms, of the mask and of its
 *                         complement, in one call);
 *       SEG_EDT_BOUNDARY  Kervadec's map as published, edt(~m) * [~m] - (edt(m) - 1) * [m]; the "- 1" is taken as written, whatever the spacing.
 * Samples without a boundary: SQUARED / DISTANCE give +inf on every voxel of a sample with no background voxel (and 0 everywhere on one with no
 * foreground); SIGNED / BOUNDARY give an all-zero map for a sample whose mask is empty OR full (Kervadec's `if posmask.any()`, extended to the full mask).
 * out: f32, sample s at out + s * out_stride_n, d*h*w values each; out_stride_n >= d*h*w is the number of floats between consecutive samples, so class k
 * of every sample can be written straight into plane k of an [n][c][d*h*w] tensor.  Nothing else of `out` is touched.
 * ws: seg_edt_ws_bytes() bytes, 256-byte aligned: 12 bytes per voxel (two value planes and the envelope stacks) + 8 bytes per 64-voxel row word + 4 per sample.
 * Limits: 1 <= n <= 65535, 1 <= d, h, w <= 2048, d*h*w < 2^31, cls -1..255, finite spacings > 0.
 *
 * seg_boundary_loss.  logits, dist: f32 [n][c][v].  p = sigmoid (c == 1) or softmax over c (c > 1) of the logits in f32;
 * out1[0] = (1 / M) * sum over samples, planes k >= first_class and voxels of p * dist, M = n * (c - first_class) * v (the mean over the selected planes:
 * SurfaceLoss with idc = range(first_class, c)).  The products are accumulated in double in a fixed order (per-workgroup partials, then one fold in
 * index order).  dlogits: NULL, or [n][c][v] that receives grad_scale * d loss / d logit, the Jacobian of the sigmoid / softmax included, in the same
 * pass: c == 1: p (1 - p) dist / M;  c > 1: p_j ([j >= first_class] dist_j - sum_{k >= first_class} p_k dist_k) / M.
 * ws: seg_boundary_loss_ws_bytes() bytes.  Limits: n >= 1, v >= 1, 1 <= c <= 16, 0 <= first_class < c.
 *
 * Both calls: stream-ordered, no allocation, no host synchronisation, no grid that depends on the data, no floating-point atomics - two calls on the same
 * input agree bit for bit.  Errors (nothing is launched, seg_last_error() says which): null pointers (dlogits excepted), limits, a spacing that is not a
 * finite positive number, an unknown mode, out_stride_n < d*h*w. */
enum { SEG_EDT_SQUARED = 0, SEG_EDT_DISTANCE = 1, SEG_EDT_SIGNED = 2, SEG_EDT_BOUNDARY = 3 };
long long seg_edt_ws_bytes(int n, int d, int h, int w);
int seg_edt(const unsigned char* labels, int n, int d, int h, int w, int cls, double sz, double sy, double sx, int mode, void* ws,
            float* out, long long out_stride_n, void* stream);
long long seg_boundary_loss_ws_bytes(int n, int c, long long v);
int seg_boundary_loss(const float* logits, const float* dist, int n, int c, long long v, int first_class, float grad_scale, void* ws,
                      float* out1, float* dlogits, void* stream);

/* ---- measurement: HIP-event timing of kernel classes inside a running forward/backward.
 * seg_profile_enable(h, mask): from now on every launch whose class bit is set in `mask` is
 * bracketed by hipEventRecord on the launch stream (0 disables).  seg_profile_read(h, ...)
 * synchronises the recorded events, returns per class {launch count, total ms, algorithmic bytes,
 * algorithmic flops} accumulated since the last read, and clears the records. */
enum {
    SEG_K_CONV3 = 0,          /* halo-tile 3^d conv, forward + data-gradient, big-box tiling of the wide levels with >= 32 channels */
    SEG_K_WGRAD3 = 1,         /* halo-tile weight gradient (main kernel + partial reduce) */
    SEG_K_CONV_GENERIC = 2,   /* gather / scatter implicit GEMM */
    SEG_K_WGRAD_GENERIC = 3,
    SEG_K_STEM = 4,
    SEG_K_GN_ACT = 5,
    SEG_K_GN_BWD_REDUCE = 6,
    SEG_K_GN_BWD_APPLY = 7,
    SEG_K_HEAD = 8,
    SEG_K_CONV3_SB = 9,       /* every other halo-tile conv (16-channel top level, deep levels) */
    SEG_K_GN_GROUP = 10,      /* one-launch GroupNorm passes of the small tensors (forward and backward) */
    SEG_K_MISC = 11,          /* everything else of a train step: fill + ingest, loss reduce / finalize / backward, fused optimiser, weight re-pack */
    SEG_K_CLS_HEAD = 12,      /* classification head (SEG_NET_RESNET): pooling, the two FC layers, their backward */
    SEG_K_COUNT = 13
};
int seg_profile_enable(seg_handle h, unsigned mask);
int seg_profile_read(seg_handle h, int* calls, float* ms, double* bytes, double* flops);

const char* seg_last_error(void);
const char* seg_build_info(void);

#ifdef __cplusplus
}
#endif
#endif

// The stateless entry points of include/segengine.h: losses, metrics, optimiser, pre / post-processing and the operator-level seg_op_* calls the
// tests and tools use.  Nothing here touches an engine handle.
#include <cmath>

#include "engine_internal.h"

// the status of an entry point that ends in a launch
#define SEG_OK(what) (hipGetLastError() == hipSuccess ? 0 : fail(what ": launch failed"))

extern "C" {

long long seg_loss_ws_bytes(int n, int c) { return (long long)align_up(loss_sums_count(n, c) * sizeof(double) * STAT_REP); }

}  // extern "C"
namespace segi {
int fill_loss(LossArgs& a, const float* logits, const void* target, int label_type, int n, int c, long long v,
                     int loss_kind, float focal_alpha, float focal_gamma, void* ws) {
    if (!logits || !target || !ws) return fail("loss: null pointer");
    if (c < 1 || c > 16) return fail("loss: classes must be 1..16");
    if (loss_kind < 0 || loss_kind >= L_KIND_COUNT) return fail("loss: unknown loss kind");
    const bool binary_kind = loss_kind <= SEG_LOSS_BINARY_CE_DICE || (loss_kind >= L_BIN_JACCARD && loss_kind <= L_BIN_TVERSKY) || loss_kind == L_BIN_SS ||
                             loss_kind == L_BIN_MCC;
    if ((c == 1) != binary_kind) return fail("loss: binary losses need C == 1, multi-class losses C > 1");
    a.logits = logits; a.target = target; a.label_type = label_type; a.N = n; a.C = c; a.V = v; a.kind = loss_kind;
    a.focal_alpha = focal_alpha; a.focal_gamma = focal_gamma; a.class_alpha = nullptr; a.sums = (double*)ws;
    a.out = nullptr; a.dlogits = nullptr; a.grad_scale = 1.f; a.phase = 0; a.n_global = 0;
    return 0;
}
}  // namespace segi
extern "C" {

int seg_loss_forward(const float* logits, const void* target, int label_type, int n, int c, long long v, int loss_kind,
                     float focal_alpha, float focal_gamma, const float* class_alpha, void* ws, float* out3, void* stream) {
    LossArgs a;
    if (fill_loss(a, logits, target, label_type, n, c, v, loss_kind, focal_alpha, focal_gamma, ws)) return -1;
    if (!out3) return fail("seg_loss_forward: out3 is null");
    a.class_alpha = class_alpha; a.out = out3;
    launch_loss_forward(a, (hipStream_t)stream);
    return SEG_OK("seg_loss_forward");
}

int seg_loss_shared_doubles(void) { return loss_shared_count(); }

int seg_loss_reduce(const float* logits, const void* target, int label_type, int n, int c, long long v, int loss_kind,
                    float focal_alpha, float focal_gamma, void* ws, void* stream) {
    LossArgs a;
    if (fill_loss(a, logits, target, label_type, n, c, v, loss_kind, focal_alpha, focal_gamma, ws)) return -1;
    a.phase = 1;
    launch_loss_forward(a, (hipStream_t)stream);
    return SEG_OK("seg_loss_reduce");
}

int seg_loss_finalize(const float* logits, const void* target, int label_type, int n, int c, long long v, int loss_kind,
                      float focal_alpha, float focal_gamma, const float* class_alpha, int n_global, void* ws, float* out3, void* stream) {
    LossArgs a;
    if (fill_loss(a, logits, target, label_type, n, c, v, loss_kind, focal_alpha, focal_gamma, ws)) return -1;
    if (!out3) return fail("seg_loss_finalize: out3 is null");
    if (n_global != 0 && n_global < n) return fail("seg_loss_finalize: n_global must be >= the local sample count (or 0: the exchanged count)");
    a.class_alpha = class_alpha; a.out = out3; a.phase = 2; a.n_global = n_global;
    launch_loss_forward(a, (hipStream_t)stream);
    return SEG_OK("seg_loss_finalize");
}

int seg_loss_backward(const float* logits, const void* target, int label_type, int n, int c, long long v, int loss_kind,
                      float focal_alpha, float focal_gamma, void* ws, float grad_scale, float* dlogits, void* stream) {
    LossArgs a;
    if (fill_loss(a, logits, target, label_type, n, c, v, loss_kind, focal_alpha, focal_gamma, ws)) return -1;
    if (!dlogits) return fail("seg_loss_backward: dlogits is null");
    a.dlogits = dlogits; a.grad_scale = grad_scale;
    launch_loss_backward(a, (hipStream_t)stream);
    return SEG_OK("seg_loss_backward");
}

long long seg_lovasz_ws_bytes(int n, long long v) {
    if (n < 1 || v < 1) return fail("seg_lovasz_ws_bytes: empty batch");
    const long long b = lovasz_ws_bytes((long long)n * v);
    return b < 0 ? fail("seg_lovasz_ws_bytes: element count must be below 2^32 (and the sort library must be usable)") : b;
}
int seg_lovasz_forward(const float* x, const void* target, int label_type, int n, int c, long long v, void* ws, float* out1, float* dx,
                       void* stream) {
    if (!x || !target || !ws || !out1 || !dx) return fail("seg_lovasz_forward: null pointer");
    if (n < 1 || v < 1 || c < 1 || c > 16) return fail("seg_lovasz_forward: classes must be 1..16, batch and volume non-empty");
    if ((long long)n * v >= (1ll << 32)) return fail("seg_lovasz_forward: element count must be below 2^32");
    if (launch_lovasz(x, target, label_type, n, c, v, ws, out1, dx, (hipStream_t)stream)) return fail("seg_lovasz_forward: sort / scan failed");
    return SEG_OK("seg_lovasz_forward");
}

static int ssim_check(const char* what, const void* a, const void* b, const void* ws, int n, int c, int d, int h, int w, int nd, int window) {
    if (!a || !b || !ws) return fail(std::string(what) + ": null pointer");
    if (n < 1 || n > 64 || c < 1 || h < 1 || w < 1 || (nd != 2 && nd != 3) || (nd == 3 && d < 1)) return fail(std::string(what) + ": bad extents (batch 1..64)");
    if (window < 1 || window > 15 || !(window & 1)) return fail(std::string(what) + ": window_size must be odd and <= 15");
    return 0;
}
long long seg_ssim_ws_bytes(int n, int c, long long v) { return (n < 1 || c < 1 || v < 1) ? -1 : ssim_ws_bytes(n * c, v); }
int seg_ssim_forward(const float* img1, const float* img2, int n, int c, int d, int h, int w, int nd, int window, void* ws, float* out,
                     void* stream) {
    if (ssim_check("seg_ssim_forward", img1, img2, ws, n, c, d, h, w, nd, window) || !out) return out ? -1 : fail("seg_ssim_forward: out is null");
    if (launch_ssim_forward(img1, img2, n, c, nd == 3 ? d : 1, h, w, nd, window, ws, out, (hipStream_t)stream)) return fail("seg_ssim_forward: bad arguments");
    return SEG_OK("seg_ssim_forward");
}
int seg_ssim_forward_cols(const float* img1, const float* img2, int n, int c, int d, int h, int w, int nd, int window, void* ws, float* out,
                          float* out_cols, void* stream) {
    if (ssim_check("seg_ssim_forward_cols", img1, img2, ws, n, c, d, h, w, nd, window) || !out || !out_cols)
        return (out && out_cols) ? -1 : fail("seg_ssim_forward_cols: out is null");
    if (launch_ssim_forward(img1, img2, n, c, nd == 3 ? d : 1, h, w, nd, window, ws, out, (hipStream_t)stream, out_cols))
        return fail("seg_ssim_forward_cols: bad arguments");
    return SEG_OK("seg_ssim_forward_cols");
}
int seg_ssim_backward(const float* img1, const float* img2, int n, int c, int d, int h, int w, int nd, int window, void* ws, const float* gscale,
                      int per_sample, float* dimg1, float* dimg2, void* stream) {
    if (ssim_check("seg_ssim_backward", img1, img2, ws, n, c, d, h, w, nd, window)) return -1;
    if (!gscale || (!dimg1 && !dimg2)) return fail("seg_ssim_backward: null pointer");
    if (launch_ssim_backward(img1, img2, n, c, nd == 3 ? d : 1, h, w, nd, window, ws, gscale, per_sample, dimg1, dimg2, (hipStream_t)stream))
        return fail("seg_ssim_backward: bad arguments");
    return SEG_OK("seg_ssim_backward");
}

int seg_predict_mask(const float* probs, unsigned char* mask, int n, int c, long long v, float threshold, int scale, void* stream) {
    if (!probs || !mask) return fail("seg_predict_mask: null pointer");
    if (c < 1 || n < 1 || v < 1 || scale < 0 || scale > 255) return fail("seg_predict_mask: bad arguments");
    launch_mask(probs, mask, n, c, v, threshold, scale, (hipStream_t)stream);
    return SEG_OK("seg_predict_mask");
}
int seg_op_resample3d(const void* src, void* dst, int elem_type, int sd, int sh, int sw, int dd, int dh, int dw, double step_z, double step_y,
                      double step_x, int mode, void* stream) {
    if (!src || !dst) return fail("seg_op_resample3d: null pointer");
    if (sd < 1 || sh < 1 || sw < 1 || dd < 1 || dh < 1 || dw < 1) return fail("seg_op_resample3d: empty volume");
    if (elem_type != 0 && elem_type != 1) return fail("seg_op_resample3d: elem_type must be 0 (f32) or 1 (u8)");
    if (mode != RS_LINEAR && mode != RS_NEAREST) return fail("seg_op_resample3d: mode must be 0 (linear) or 1 (nearest)");
    if (mode == RS_LINEAR && elem_type != 0) return fail("seg_op_resample3d: linear interpolation needs f32 volumes");
    if (!(step_z > 0.0) || !(step_y > 0.0) || !(step_x > 0.0)) return fail("seg_op_resample3d: steps must be positive");
    ResampleArgs a;
    a.src = src; a.dst = dst; a.sD = sd; a.sH = sh; a.sW = sw; a.dD = dd; a.dH = dh; a.dW = dw;
    a.fz = step_z; a.fy = step_y; a.fx = step_x; a.mode = mode;
    launch_resample3d(a, elem_type, (hipStream_t)stream);
    return SEG_OK("seg_op_resample3d");
}
long long seg_op_normalize_ws_bytes(void) { return (long long)normalize_ws_bytes(); }
int seg_op_normalize_meanstd(const float* x, float* out, long long n, int clip, float lower, float upper, void* ws, void* stream) {
    if (!x || !out || !ws) return fail("seg_op_normalize_meanstd: null pointer");
    if (n < 1) return fail("seg_op_normalize_meanstd: empty volume");
    if (clip && !(lower <= upper)) return fail("seg_op_normalize_meanstd: lower > upper");
    launch_normalize_meanstd(x, out, n, clip, lower, upper, ws, (hipStream_t)stream);
    return SEG_OK("seg_op_normalize_meanstd");
}
int seg_op_normalize_percentile(const float* x, float* out, long long n, float q_lo, float q_hi, void* ws, void* stream) {
    if (!x || !out || !ws) return fail("seg_op_normalize_percentile: null pointer");
    if (n < 1) return fail("seg_op_normalize_percentile: empty volume");
    if (!(q_lo >= 0.f && q_lo <= q_hi && q_hi <= 100.f)) return fail("seg_op_normalize_percentile: need 0 <= q_lo <= q_hi <= 100");
    launch_normalize_percentile(x, out, n, q_lo, q_hi, ws, (hipStream_t)stream);
    return SEG_OK("seg_op_normalize_percentile");
}
static int check_windows(const char* what, int D, int H, int W, int nb, int pd, int ph, int pw) {
    if (nb < 1 || pd < 1 || ph < 1 || pw < 1) return fail(std::string(what) + ": empty patch list");
    if (pd > D || ph > H || pw > W) return fail(std::string(what) + ": patch larger than the volume");
    return 0;
}
int seg_op_gather_patches(const float* vol, int d, int h, int w, const int* origins, int nb, int pd, int ph, int pw, float* out, void* stream) {
    if (!vol || !origins || !out) return fail("seg_op_gather_patches: null pointer");
    if (check_windows("seg_op_gather_patches", d, h, w, nb, pd, ph, pw)) return -1;
    launch_gather_patches(vol, d, h, w, origins, nb, pd, ph, pw, out, (hipStream_t)stream);
    return SEG_OK("seg_op_gather_patches");
}
int seg_op_stitch_mask(const unsigned char* masks, const int* origins, int nb, int pd, int ph, int pw, unsigned char* out, int d, int h, int w,
                       void* stream) {
    if (!masks || !origins || !out) return fail("seg_op_stitch_mask: null pointer");
    if (check_windows("seg_op_stitch_mask", d, h, w, nb, pd, ph, pw)) return -1;
    launch_stitch_mask(masks, origins, nb, pd, ph, pw, out, d, h, w, (hipStream_t)stream);
    return SEG_OK("seg_op_stitch_mask");
}
int seg_op_gather_windows(const float* vol, int d, int h, int w, const int* entries, int nb, int pd, int ph, int pw, float pad_value, float* out,
                          void* stream) {
    if (!vol || !entries || !out) return fail("seg_op_gather_windows: null pointer");
    if (d < 1 || h < 1 || w < 1) return fail("seg_op_gather_windows: empty volume");
    if (nb < 1 || pd < 1 || ph < 1 || pw < 1) return fail("seg_op_gather_windows: empty window list");
    launch_gather_windows(vol, d, h, w, entries, nb, pd, ph, pw, pad_value, out, (hipStream_t)stream);
    return SEG_OK("seg_op_gather_windows");
}
int seg_op_blend_windows(const float* probs, const int* entries, int nb, int c, int pd, int ph, int pw, const float* wz, const float* wy,
                         const float* wx, const int* box_lo, const int* box_hi, float* acc, float* wsum, int d, int h, int w, void* stream) {
    if (!probs || !entries || !wz || !wy || !wx || !box_lo || !box_hi || !acc || !wsum) return fail("seg_op_blend_windows: null pointer");
    if (d < 1 || h < 1 || w < 1) return fail("seg_op_blend_windows: empty volume");
    if (nb < 1 || pd < 1 || ph < 1 || pw < 1) return fail("seg_op_blend_windows: empty window list");
    if (c < 1 || c > 16) return fail("seg_op_blend_windows: classes must be 1..16");
    const int dims[3] = {d, h, w};
    for (int a = 0; a < 3; ++a)
        if (box_lo[a] < 0 || box_hi[a] > dims[a] || box_lo[a] >= box_hi[a]) return fail("seg_op_blend_windows: the box must be non-empty and inside the volume");
    launch_blend_windows(probs, entries, nb, c, pd, ph, pw, wz, wy, wx, box_lo, box_hi, acc, wsum, d, h, w, (hipStream_t)stream);
    return SEG_OK("seg_op_blend_windows");
}
int seg_op_blend_finalize(const float* acc, const float* wsum, int c, long long v, float threshold, int scale, unsigned char* mask, float* probs_out,
                          void* stream) {
    if (!acc || !wsum || !mask) return fail("seg_op_blend_finalize: null pointer");
    if (c < 1 || c > 16) return fail("seg_op_blend_finalize: classes must be 1..16");
    if (v < 1 || scale < 0 || scale > 255) return fail("seg_op_blend_finalize: empty volume or scale outside 0..255");
    launch_blend_finalize(acc, wsum, c, v, threshold, scale, mask, probs_out, (hipStream_t)stream);
    return SEG_OK("seg_op_blend_finalize");
}

int seg_metric(const float* probs, const void* target, int label_type, int n, int c, long long v, void* ws, float* out2, void* stream) {
    if (!probs || !target || !ws || !out2) return fail("seg_metric: null pointer");
    if (c < 1 || c > 16) return fail("seg_metric: classes must be 1..16");
    launch_metric(probs, target, label_type, n, c, v, (double*)ws, out2, (hipStream_t)stream);
    return SEG_OK("seg_metric");
}


static int surface_extents_ok(int d, int h, int w) {
    return d >= 1 && h >= 1 && w >= 1 && d <= 2048 && h <= 2048 && w <= 2048 && (long long)d * h * w < (1ll << 31);
}
long long seg_surface_ws_bytes(int d, int h, int w) {
    if (!surface_extents_ok(d, h, w)) return fail("seg_surface_ws_bytes: extents must be 1..2048 with d*h*w < 2^31");
    return (long long)surface_ws_bytes(d, h, w);
}
int seg_surface_metrics(const unsigned char* real, const unsigned char* pred, int d, int h, int w, int cls, double sz, double sy, double sx, void* ws,
                        double* out16, float* real2pred_nn, float* pred2real_nn, void* stream) {
    if (!real || !pred || !ws || !out16) return fail("seg_surface_metrics: null pointer");
    if (!surface_extents_ok(d, h, w)) return fail("seg_surface_metrics: extents must be 1..2048 with d*h*w < 2^31");
    if (cls < -1 || cls > 255) return fail("seg_surface_metrics: cls must be -1 (label != 0) or a label value 0..255");
    launch_surface_metrics(real, pred, d, h, w, cls, sz, sy, sx, ws, out16, real2pred_nn, pred2real_nn, (hipStream_t)stream);
    return SEG_OK("seg_surface_metrics");
}


static int augment_extents_ok(int n, int c, int n0, int n1, int n2) {
    return n >= 1 && n <= 65535 && c >= 1 && c <= 65535 && n0 >= 1 && n1 >= 1 && n2 >= 1 && (long long)n0 * n1 <= (1ll << 31) &&
           (long long)n0 * n1 * n2 <= (1ll << 31);
}
// the last element of a sample, (c - 1)*xs_c + (V - 1)*xs_v, lies inside its c*V elements: (V, 1), (1, c) and nothing that reaches further
static int augment_strides_ok(int c, long long V, long long xs_c, long long xs_v) {
    return xs_c >= 1 && xs_v >= 1 && xs_c <= V && xs_v <= c && (c - 1) * xs_c + (V - 1) * xs_v < (long long)c * V;
}
long long seg_augment3d_ws_bytes(int n) {
    if (n < 1 || n > 65535) return fail("seg_augment3d_ws_bytes: n must be 1..65535");
    return (long long)augment3d_ws_bytes(n);
}
int seg_augment3d(const float* x, float* out, int n, int c, int n0, int n1, int n2, long long xs_c, long long xs_v, const void* label, void* label_out,
                  int label_type, int label_c, const double* params_host, const double* params_dev, int fill_mode, double cval, double label_cval,
                  double rescale, int extrema, void* ws, void* stream) {
    if (!x || !out || x == out || !params_host || !params_dev || !ws || (label != nullptr) != (label_out != nullptr) || (label && label == label_out))
        return fail("seg_augment3d: null pointer, or a transform in place");
    if (!augment_extents_ok(n, c, n0, n1, n2)) return fail("seg_augment3d: n, c must be 1..65535, extents >= 1 with n0*n1*n2 <= 2^31");
    if (!augment_strides_ok(c, (long long)n0 * n1 * n2, xs_c, xs_v)) return fail("seg_augment3d: strides must be positive and stay inside a sample's c*V elements");
    if (fill_mode == SEG_AUGMENT_REFLECT || fill_mode == SEG_AUGMENT_WRAP)
        return fail("seg_augment3d: fill modes reflect and wrap are not implemented (nearest and constant are)");
    if (fill_mode != SEG_AUGMENT_NEAREST && fill_mode != SEG_AUGMENT_CONSTANT) return fail("seg_augment3d: unknown fill mode");
    if (label && label_type != LT_U8 && label_type != LT_I64 && label_type != LT_F32) return fail("seg_augment3d: label type must be u8, i64 or f32");
    if (label && label_c != 1 && label_c != c) return fail("seg_augment3d: label_c must be 1 or c");
    if (extrema && c > 8) return fail("seg_augment3d: a channel shift needs c <= 8");
    if (!std::isfinite(cval) || !std::isfinite(label_cval) || !std::isfinite(rescale)) return fail("seg_augment3d: cval / rescale must be finite");
    for (int s = 0; s < n; ++s) {
        const double* p = params_host + (size_t)s * SEG_AUGMENT_PARAM_DOUBLES;
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(p[k])) return fail("seg_augment3d: non-finite matrix or offset");
        if (!(p[12] >= 0.0 && p[12] <= 7.0) || p[12] != (double)(int)p[12]) return fail("seg_augment3d: flips must be an integer 0..7");
    }
    if (label && fill_mode == SEG_AUGMENT_CONSTANT && label_type != LT_F32) {
        const double lim = label_type == LT_U8 ? 255.0 : 9007199254740992.0;      // (2^53: every integer below is a double)
        if (label_cval != std::floor(label_cval) || label_cval > lim || label_cval < (label_type == LT_U8 ? 0.0 : -lim))
            return fail("seg_augment3d: label_cval is not representable in the label type");
    }
    Augment3dArgs a = {};
    a.x = x; a.out = out; a.label = label; a.label_out = label_out; a.params = params_dev;
    a.N = n; a.C = c; a.LC = label ? label_c : 0; a.n0 = n0; a.n1 = n1; a.n2 = n2;
    a.V = (long long)n0 * n1 * n2; a.xs_c = xs_c; a.xs_v = xs_v;
    a.ls_c = label_c == 1 ? 0 : xs_c; a.ls_v = label_c == 1 ? 1 : xs_v;
    a.constant = fill_mode == SEG_AUGMENT_CONSTANT; a.cval = (float)cval; a.label_cval = label_cval;
    a.extrema = extrema != 0;
    a.has_scale = !a.extrema && rescale != 0.0; a.scale = (float)rescale;
    launch_augment3d(a, label_type, ws, (hipStream_t)stream);
    return SEG_OK("seg_augment3d");
}
int seg_augment3d_shift(float* x, int n, int c, int n0, int n1, int n2, long long xs_c, long long xs_v, const double* params_dev, double rescale,
                        const void* ws, void* stream) {
    if (!x || (params_dev && !ws)) return fail("seg_augment3d_shift: null pointer");
    if (!augment_extents_ok(n, c, n0, n1, n2)) return fail("seg_augment3d_shift: n, c must be 1..65535, extents >= 1 with n0*n1*n2 <= 2^31");
    if (!augment_strides_ok(c, (long long)n0 * n1 * n2, xs_c, xs_v))
        return fail("seg_augment3d_shift: strides must be positive and stay inside a sample's c*V elements");
    if (params_dev && c > 8) return fail("seg_augment3d_shift: a channel shift needs c <= 8");
    if (!std::isfinite(rescale)) return fail("seg_augment3d_shift: rescale must be finite");
    if (!params_dev && rescale == 0.0) return 0;
    launch_augment3d_shift(x, n, c, (long long)n0 * n1 * n2, xs_c, xs_v, params_dev, ws, (float)rescale, rescale != 0.0, (hipStream_t)stream);
    return SEG_OK("seg_augment3d_shift");
}

long long seg_augment2d_ws_bytes(int n) {
    if (n < 1 || n > 65535) return fail("seg_augment2d_ws_bytes: n must be 1..65535");
    return 0;
}
int seg_augment2d(const float* x, float* out, int n, int c, int h, int w, long long xs_n, long long xs_c, long long xs_v, const void* label,
                  void* label_out, int label_type, const double* params_host, const double* params_dev, int border_mode, double cval,
                  double label_cval, void* ws, void* stream) {
    (void)ws;
    if (!x || !out || x == out || !params_host || !params_dev || (label != nullptr) != (label_out != nullptr) || (label && label == label_out))
        return fail("seg_augment2d: null pointer, or a transform in place");
    if (!augment_extents_ok(n, c, 1, h, w)) return fail("seg_augment2d: n, c must be 1..65535, extents >= 1 with h*w <= 2^31");
    const long long V = (long long)h * w;
    if (!augment_strides_ok(c, V, xs_c, xs_v) || (xs_n != 0 && xs_n < (long long)c * V))
        return fail("seg_augment2d: strides must be positive and stay inside a sample's c*V elements, xs_n 0 or >= c*V");
    if (border_mode == SEG_AUGMENT_REFLECT || border_mode == SEG_AUGMENT_WRAP)
        return fail("seg_augment2d: border modes reflect and wrap are not implemented (mirror, nearest and constant are)");
    if (border_mode != SEG_AUGMENT_MIRROR && border_mode != SEG_AUGMENT_NEAREST && border_mode != SEG_AUGMENT_CONSTANT)
        return fail("seg_augment2d: unknown border mode");
    if (label && label_type != LT_U8 && label_type != LT_I64 && label_type != LT_F32) return fail("seg_augment2d: label type must be u8, i64 or f32");
    if (!std::isfinite(cval) || !std::isfinite(label_cval)) return fail("seg_augment2d: cval must be finite");
    for (int s = 0; s < n; ++s) {
        const double* p = params_host + (size_t)s * SEG_AUGMENT2D_PARAM_DOUBLES;
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(p[k])) return fail("seg_augment2d: non-finite matrix");
        if (!std::isfinite(p[10]) || !std::isfinite(p[11])) return fail("seg_augment2d: non-finite alpha or beta");
        if (!(p[6] >= 0.0 && p[6] <= 3.0) || p[6] != (double)(int)p[6]) return fail("seg_augment2d: flips must be an integer 0..3");
        if (!std::isfinite(p[7]) || !std::isfinite(p[12])) return fail("seg_augment2d: non-finite warp or clip switch");
        if (p[8] != 0.0 && p[8] != 1.0 && p[8] != 2.0) return fail("seg_augment2d: blur must be 0 (none), 1 (weights) or 2 (median)");
        if (p[8] == 1.0) {
            if (p[9] != 3.0 && p[9] != 5.0 && p[9] != 7.0) return fail("seg_augment2d: k must be 3, 5 or 7");
            for (int k = 0; k < (int)(p[9] * p[9]); ++k)
                if (!std::isfinite(p[k < 48 ? 16 + k : 15])) return fail("seg_augment2d: non-finite blur weight");
        }
        if (p[12] != 0.0 && !(p[13] <= p[14])) return fail("seg_augment2d: clip needs clip_lo <= clip_hi");
    }
    if (label && border_mode == SEG_AUGMENT_CONSTANT && label_type != LT_F32) {
        const double lim = label_type == LT_U8 ? 255.0 : 9007199254740992.0;      // (2^53: every integer below is a double)
        if (label_cval != std::floor(label_cval) || label_cval > lim || label_cval < (label_type == LT_U8 ? 0.0 : -lim))
            return fail("seg_augment2d: label_cval is not representable in the label type");
    }
    Augment2dArgs a = {};
    a.x = x; a.out = out; a.label = label; a.label_out = label_out; a.params = params_dev;
    a.N = n; a.C = c; a.H = h; a.W = w; a.V = V; a.xs_n = xs_n; a.xs_c = xs_c; a.xs_v = xs_v; a.ls_n = xs_n == 0 ? 0 : V;
    a.border = border_mode; a.cval = (float)cval; a.label_cval = label_cval;
    launch_augment2d(a, label_type, (hipStream_t)stream);
    return SEG_OK("seg_augment2d");
}


static int postproc_extents_ok(int n, int d, int h, int w) {
    return n >= 1 && n <= 65535 && d >= 1 && h >= 1 && w >= 1 && d <= 2048 && h <= 2048 && w <= 2048 && (long long)n * d * h * w < (1ll << 31);
}
static const char* const POSTPROC_EXTENTS = "n must be 1..65535, extents 1..2048 with n*d*h*w < 2^31";
long long seg_cc_ws_bytes(int n, int d, int h, int w) {
    if (!postproc_extents_ok(n, d, h, w)) return fail(std::string("seg_cc_ws_bytes: ") + POSTPROC_EXTENTS);
    return (long long)cc_ws_bytes(n, d, h, w);
}
int seg_cc_label(const unsigned char* mask, int n, int d, int h, int w, int cls, int connectivity, void* ws, int* labels, int* stats, void* stream) {
    if (!mask || !ws || !stats) return fail("seg_cc_label: null pointer");
    if (!postproc_extents_ok(n, d, h, w)) return fail(std::string("seg_cc_label: ") + POSTPROC_EXTENTS);
    if (cls < -1 || cls > 255) return fail("seg_cc_label: cls must be -1 (value != 0) or a value 0..255");
    if (connectivity != 1 && connectivity != 3) return fail("seg_cc_label: connectivity must be 1 (faces) or 3 (fully connected)");
    launch_cc_label(mask, n, d, h, w, cls, connectivity, ws, labels, stats, (hipStream_t)stream);
    return SEG_OK("seg_cc_label");
}
int seg_cc_filter(const unsigned char* mask, unsigned char* out, int n, int d, int h, int w, int cls, int connectivity, int mode, long long min_voxels,
                  void* ws, int* stats, void* stream) {
    if (!mask || !out || !ws) return fail("seg_cc_filter: null pointer");
    if (!postproc_extents_ok(n, d, h, w)) return fail(std::string("seg_cc_filter: ") + POSTPROC_EXTENTS);
    if (cls < -1 || cls > 255) return fail("seg_cc_filter: cls must be -1 (value != 0) or a value 0..255");
    if (connectivity != 1 && connectivity != 3) return fail("seg_cc_filter: connectivity must be 1 (faces) or 3 (fully connected)");
    if (mode != SEG_CC_KEEP_LARGEST && mode != SEG_CC_MIN_SIZE) return fail("seg_cc_filter: unknown mode");
    if (mode == SEG_CC_MIN_SIZE && min_voxels < 0) return fail("seg_cc_filter: min_voxels must not be negative");
    launch_cc_filter(mask, out, n, d, h, w, cls, connectivity, mode, min_voxels, ws, stats, (hipStream_t)stream);
    return SEG_OK("seg_cc_filter");
}
long long seg_morph3d_ws_bytes(int n, int d, int h, int w) {
    if (!postproc_extents_ok(n, d, h, w)) return fail(std::string("seg_morph3d_ws_bytes: ") + POSTPROC_EXTENTS);
    return (long long)morph3d_ws_bytes(n, d, h, w);
}
int seg_morph3d(const unsigned char* mask, unsigned char* out, int n, int d, int h, int w, int cls, int op, int shape, int rz, int ry, int rx, int border,
                int fg_value, void* ws, void* stream) {
    if (!mask || !out || !ws) return fail("seg_morph3d: null pointer");
    if (!postproc_extents_ok(n, d, h, w)) return fail(std::string("seg_morph3d: ") + POSTPROC_EXTENTS);
    if (cls < -1 || cls > 255) return fail("seg_morph3d: cls must be -1 (value != 0) or a value 0..255");
    if (op < SEG_MORPH_DILATE || op > SEG_MORPH_CLOSE) return fail("seg_morph3d: unknown operation");
    if (shape < SEG_SE_BALL || shape > SEG_SE_CROSS) return fail("seg_morph3d: unknown structuring element");
    if (rz < 0 || ry < 0 || rx < 0 || rz > 31 || ry > 31 || rx > 31) return fail("seg_morph3d: radii must be 0..31");
    if (border < -1 || border > 1) return fail("seg_morph3d: border must be 0, 1 or -1 (the operation's default)");
    if ((op == SEG_MORPH_OPEN || op == SEG_MORPH_CLOSE) && border != -1) return fail("seg_morph3d: open and close take no explicit border");
    if (fg_value < 0 || fg_value > 255) return fail("seg_morph3d: fg_value must be 0..255");
    launch_morph3d(mask, out, n, d, h, w, cls, op, shape, rz, ry, rx, border, fg_value, ws, (hipStream_t)stream);
    return SEG_OK("seg_morph3d");
}

static int edt_extents_ok(int n, int d, int h, int w) {
    return n >= 1 && n <= 65535 && d >= 1 && h >= 1 && w >= 1 && d <= 2048 && h <= 2048 && w <= 2048 && (long long)d * h * w < (1ll << 31);
}
static const char* const EDT_EXTENTS = "n must be 1..65535, extents 1..2048 with d*h*w < 2^31";
long long seg_edt_ws_bytes(int n, int d, int h, int w) {
    if (!edt_extents_ok(n, d, h, w)) return fail(std::string("seg_edt_ws_bytes: ") + EDT_EXTENTS);
    return (long long)edt_ws_bytes(n, d, h, w);
}
int seg_edt(const unsigned char* labels, int n, int d, int h, int w, int cls, double sz, double sy, double sx, int mode, void* ws, float* out,
            long long out_stride_n, void* stream) {
    if (!labels || !ws || !out) return fail("seg_edt: null pointer");
    if (!edt_extents_ok(n, d, h, w)) return fail(std::string("seg_edt: ") + EDT_EXTENTS);
    if (cls < -1 || cls > 255) return fail("seg_edt: cls must be -1 (label != 0) or a label value 0..255");
    const float fz = (float)sz, fy = (float)sy, fx = (float)sx;       // rounded once; what the kernels compute with
    if (!(std::isfinite(fz) && std::isfinite(fy) && std::isfinite(fx) && fz > 0.f && fy > 0.f && fx > 0.f))
        return fail("seg_edt: spacings must be finite and positive (as f32)");
    if (mode < SEG_EDT_SQUARED || mode > SEG_EDT_BOUNDARY) return fail("seg_edt: unknown mode");
    if (out_stride_n < (long long)d * h * w) return fail("seg_edt: out_stride_n must be at least d*h*w");
    launch_edt(labels, n, d, h, w, cls, fz, fy, fx, mode, ws, out, out_stride_n, (hipStream_t)stream);
    return SEG_OK("seg_edt");
}
static int boundary_loss_extents_ok(int n, int c, long long v) { return n >= 1 && v >= 1 && c >= 1 && c <= 16; }
long long seg_boundary_loss_ws_bytes(int n, int c, long long v) {
    if (!boundary_loss_extents_ok(n, c, v)) return fail("seg_boundary_loss_ws_bytes: classes must be 1..16, batch and volume non-empty");
    return (long long)boundary_loss_ws_bytes();
}
int seg_boundary_loss(const float* logits, const float* dist, int n, int c, long long v, int first_class, float grad_scale, void* ws, float* out1,
                      float* dlogits, void* stream) {
    if (!logits || !dist || !ws || !out1) return fail("seg_boundary_loss: null pointer");
    if (!boundary_loss_extents_ok(n, c, v)) return fail("seg_boundary_loss: classes must be 1..16, batch and volume non-empty");
    if (first_class < 0 || first_class >= c) return fail("seg_boundary_loss: first_class must be 0..c-1");
    if (!std::isfinite(grad_scale)) return fail("seg_boundary_loss: grad_scale must be finite");
    launch_boundary_loss(logits, dist, n, c, v, first_class, grad_scale, ws, out1, dlogits, (hipStream_t)stream);
    return SEG_OK("seg_boundary_loss");
}

}  // extern "C"
namespace segi {
// riders: the overflow flag was cleared and the step counter will be advanced by StepRiders of neighbouring launches (seg_train_step)
int adam_step_impl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long numel, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int decoupled, float inv_scale, int check_finite, int* state, void* stream,
                          bool riders) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !state) return fail("seg_adam_step: null pointer");
    hipStream_t st = (hipStream_t)stream;
    AdamArgs a;
    a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.n = numel;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.decoupled = decoupled;
    a.inv_scale = inv_scale; a.step = state; a.found_inf = state + 1;
    if (!riders) (void)hipMemsetAsync(state + 1, 0, sizeof(int), st);
    if (check_finite) launch_grad_check(grads, numel, state + 1, st);
    launch_adam(a, st, !riders);
    return SEG_OK("seg_adam_step");
}
}  // namespace segi
extern "C" {
int seg_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long numel, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int decoupled, float inv_scale, int check_finite, int* state, void* stream) {
    return adam_step_impl(params, grads, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, decoupled, inv_scale, check_finite, state,
                          stream, false);
}

int seg_op_conv(const seg_conv_args* a, int dtype, void* stream) {
    if (!a || !a->in0 || !a->w || !a->out) return fail("seg_op_conv: null pointer");
    const int cin = a->C0 + a->C1;
    if (cin < 8 || (cin & (cin - 1)) || a->C0 % 8) return fail("seg_op_conv: channel counts must be powers of two >= 8");
    if (a->Cout % 16 || a->Ngemm % 16 || a->Kpad % 32 || a->Kpad < a->K) return fail("seg_op_conv: bad GEMM extents");
    if ((a->act_scale || a->act_shift) && !(a->act_scale && a->act_shift && conv_uses_stream_kernel(*a)))
        return fail("seg_op_conv: act_scale / act_shift need the streaming kernel (gather form, seg_op_conv_kernel == 1) and come as a pair");
    if (a->rq_Q && !(a->out1 && conv_uses_stream_kernel(*a))) return fail("seg_op_conv: rq_* need out1 / Cout0 on the streaming kernel and all of rq_r, rq_scale, rq_shift");
    if (a->out1 && !conv_uses_stream_kernel(*a)) return fail("seg_op_conv: out1 / Cout0 need the streaming kernel (gather form, no bias / stats, 16-channel tiles in pairs)");
    launch_conv_igemm(*a, dtype, (hipStream_t)stream);
    return SEG_OK("seg_op_conv");
}
int seg_op_conv_kernel(const seg_conv_args* a) { return a ? (conv_uses_stream_kernel(*a) ? 1 : 0) : -1; }
long long seg_op_wgrad_partial_bytes(const seg_wgrad_args* a) { return a ? (long long)wgrad_partial_bytes(*a) : -1; }
int seg_op_wgrad(const seg_wgrad_args* a, float* partial_scratch, int dtype, void* stream) {
    if (!a || !a->dr || !a->x0 || !a->dw || !partial_scratch) return fail("seg_op_wgrad: null pointer");
    if (a->P % 16) return fail("seg_op_wgrad: P must be a multiple of 16");
    if (a->stem ? (a->Q > 32) : (a->Q % 16 != 0)) return fail("seg_op_wgrad: bad Q");
    if ((a->act_scale || a->act_shift) && !(a->act_scale && a->act_shift && dtype != SEG_F32 && wgrad_act_supported(*a)))
        return fail("seg_op_wgrad: act_scale / act_shift need a 1^d stride-1 conv on 16-bit tensors with C0 <= 64 and come as a pair");
    launch_wgrad(*a, partial_scratch, dtype, (hipStream_t)stream);
    return SEG_OK("seg_op_wgrad");
}
int seg_op_wgrad_kernel(const seg_wgrad_args* a, int dtype) { return a ? wgrad_kernel_id(*a, dtype) : -1; }
int seg_op_pack(const seg_pack_desc* descs, int ndesc, long long max_elems, int dtype, void* stream) {
    if (!descs || ndesc < 1) return fail("seg_op_pack: no descriptors");
    launch_pack(descs, ndesc, (int)max_elems, dtype, (hipStream_t)stream);
    return SEG_OK("seg_op_pack");
}
int seg_op_conv3(const void* in, const void* w, const float* bias, void* out, double* stats, int n, int d, int h, int wid, int cin,
                 int cout, int ndim, int dtype, void* stream) {
    if (!in || !w || !out) return fail("seg_op_conv3: null pointer");
    if (cin < 16 || (cin & (cin - 1)) || cout % 16) return fail("seg_op_conv3: Cin must be a power of two >= 16, Cout a multiple of 16");
    launch_conv3(in, w, bias, out, stats, n, ndim == 3 ? d : 1, h, wid, cin, cout, ndim, dtype, (hipStream_t)stream);
    return SEG_OK("seg_op_conv3");
}
int seg_op_conv3x(int cfg, const void* in0, const void* in1, int c0, const void* w, const float* bias, void* out, double* stats, int n, int d,
                  int h, int wid, int cin, int cout, int ndim, int dtype, void* stream) {
    if (!in0 || !w || !out) return fail("seg_op_conv3x: null pointer");
    if (ndim != 2 && ndim != 3) return fail("seg_op_conv3x: ndim must be 2 or 3");
    const int dd = ndim == 3 ? d : 1;
    if (!conv3x_supported(dtype, ndim, n, dd, h, wid, cin, cout, c0, in1 != nullptr))
        return fail("seg_op_conv3x: needs a 16-bit dtype, Cin % 32 == 0 (or Cin == 16 without a concat), Cout % 16 == 0 and tensors below 2 GB per sample");
    if (cfg < 0) cfg = conv3x_pick(ndim, n, dd, h, wid, cin, cout);
    if (cfg < 0 || !launch_conv3x(cfg, in0, in1, c0, w, bias, out, stats, n, dd, h, wid, cin, cout, ndim, dtype, (hipStream_t)stream))
        return fail("seg_op_conv3x: the tiling does not fit this shape");
    return SEG_OK("seg_op_conv3x");
}
int seg_op_conv3x_num_cfgs(void) { return conv3x_num_cfgs(); }
int seg_op_conv3x_cfg_frag(int cfg) { return conv3x_cfg_frag(cfg); }
int seg_op_conv3x_cfg_info(int index, int* id, int* ndim, int* box3, int* bn, int* nres, char* name, int name_cap) {
    const char* nm = nullptr;
    if (conv3x_cfg_info(index, id, ndim, box3, bn, nres, &nm)) return fail("seg_op_conv3x_cfg_info: index out of range");
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", nm);
    return 0;
}
int seg_op_conv3x_default_cfg(int ndim, int n, int d, int h, int wid, int cin, int cout, int dtype) {
    const int dd = ndim == 3 ? d : 1;
    if (!conv3x_supported(dtype, ndim, n, dd, h, wid, cin, cout, 0, false)) return -1;
    return conv3x_pick(ndim, n, dd, h, wid, cin, cout);
}
long long seg_op_wgrad3_partial_bytes(int ndim, int n, int d, int h, int wid, int p, int q) {
    return (long long)wgrad3_partial_bytes(ndim, n, ndim == 3 ? d : 1, h, wid, p, q);
}
int seg_op_wgrad3(const void* dr, const void* x, float* partial, float* dw, int n, int d, int h, int wid, int p, int q, int ndim,
                  int dtype, void* stream) {
    if (!dr || !x || !partial || !dw) return fail("seg_op_wgrad3: null pointer");
    if (p % 16 || q % 16 || (p > 16 && p % 32) || (q > 16 && q % 32)) return fail("seg_op_wgrad3: channel counts must be 16 or multiples of 32");
    launch_wgrad3(dr, x, partial, dw, n, ndim == 3 ? d : 1, h, wid, p, q, ndim, dtype, (hipStream_t)stream);
    return SEG_OK("seg_op_wgrad3");
}
int seg_op_wgrad3_cat(const void* dr, const void* x0, const void* x1, int c0, float* partial, float* dw, int n, int d, int h, int wid, int p,
                      int q, int ndim, int dtype, void* stream) {
    if (!dr || !x0 || !x1 || !partial || !dw) return fail("seg_op_wgrad3_cat: null pointer");
    if (p % 16 || q % 16 || (p > 16 && p % 32) || (q > 16 && q % 32)) return fail("seg_op_wgrad3_cat: channel counts must be 16 or multiples of 32");
    if (c0 <= 0 || c0 >= q || c0 % 16) return fail("seg_op_wgrad3_cat: c0 must be a multiple of 16 inside (0, q)");
    launch_wgrad3(dr, x0, partial, dw, n, ndim == 3 ? d : 1, h, wid, p, q, ndim, dtype, (hipStream_t)stream, x1, c0);
    return SEG_OK("seg_op_wgrad3_cat");
}
long long seg_op_stemx_partial_bytes(int ndim, int n, int d, int h, int wid, int cimg) {
    return (long long)stemx_partial_bytes(ndim, n, ndim == 3 ? d : 1, h, wid, cimg);
}
long long seg_op_stemx_moment_bytes(int ndim, int n, int d, int h, int wid, int cimg) {
    if (n < 1 || cimg < 1) return 0;
    return (long long)stemx_moment_bytes(ndim, n, ndim == 3 ? d : 1, h, wid, cimg);
}
int seg_op_stemx(const seg_stemx_args* a, int mode, int ndim, int dtype, float* dw3, float* dw1, void* stream) {
    if (!a || !a->img || !a->w3) return fail("seg_op_stemx: null pointer");
    if (mode < 0 || mode > 5) return fail("seg_op_stemx: mode must be 0..5");
    if (a->N < 1) return fail("seg_op_stemx: batch must be >= 1");
    if (ndim != 2 && ndim != 3) return fail("seg_op_stemx: ndim must be 2 or 3");
    if (a->Cimg < 1 || a->Cimg > 3 || (ndim == 3 && a->Cimg != 1)) return fail("seg_op_stemx: image channels must be 1 (3-D) or 1..3 (2-D)");
    if ((long long)(ndim == 3 ? a->D : 1) * a->H * a->W * 16 * 4 >= (1ll << 31)) return fail("seg_op_stemx: volume too large for one buffer range");
    if (mode == 0 && (!a->stats3 || (a->w1 && !a->stats1))) return fail("seg_op_stemx: statistics pointers");
    if (mode >= 1 && mode != 5 && (!a->scale3 || !a->shift3 || (a->w1 && (!a->scale1 || !a->shift1)))) return fail("seg_op_stemx: scale / shift pointers");
    if (mode == 1 && !a->out) return fail("seg_op_stemx: out is null");
    if (mode >= 2 && mode != 5 && (a->ndy < 1 || a->ndy > 3 || !a->dy[0])) return fail("seg_op_stemx: gradient sources");
    if ((mode == 2 || mode == 4) && (!a->Q3 || (a->w1 && !a->Q1))) return fail("seg_op_stemx: Q pointers");
    if (mode == 4 && !a->partial) return fail("seg_op_stemx: moment scratch is null");
    if ((mode == 3 || mode == 5) && (!a->coef3 || (a->w1 && !a->coef1) || !a->partial || !dw3 || (a->w1 && !dw1))) return fail("seg_op_stemx: weight-gradient pointers");
    launch_stemx(*a, mode, ndim, dtype, dw3, dw1, (hipStream_t)stream);
    return SEG_OK("seg_op_stemx");
}
int seg_abi_sizeof(int which) {
    return which == 0 ? (int)sizeof(seg_conv_args) : which == 1 ? (int)sizeof(seg_wgrad_args) : which == 2 ? (int)sizeof(seg_pack_desc)
           : which == 3 ? (int)sizeof(seg_stemx_args) : which == 5 ? (int)sizeof(seg_gn_fwd_args) : which == 6 ? (int)sizeof(seg_gn_bwd_args)
           : (int)sizeof(seg_train_args);
}

// ---- GroupNorm + dropout + ReLU and max-pool at operator level: the engine's launches (engine_plan.hip: fwd_act, bwd_act, bwd_act_dual) with the path
// named by the caller
}  // extern "C"
namespace segi {
static const char* gn_shape_error(int N, int C, long long V, int dtype) {
    if (dtype < DT_F32 || dtype > DT_BF16) return "unknown dtype";
    if (C != 16 && C != 32 && C != 64 && C != 128 && C != 256) return "C must be 16, 32, 64, 128 or 256";
    if (N < 1 || N > 65535 || V < 1) return "N must be 1..65535 and V >= 1";
    if (V * (C / 8) >= (1ll << 31) || (long long)N * V * (C / 8) >= (1ll << 31)) return "tensor too large (chunk index in 32 bits)";
    return nullptr;
}
}  // namespace segi
extern "C" {
int seg_op_gn_forward(const seg_gn_fwd_args* a, int dtype, void* stream) {
    if (!a || !a->r1 || !a->out || !a->stats1 || !a->gamma1 || !a->beta1 || !a->scale1 || !a->shift1 || !a->mean1 || !a->rstd1)
        return fail("seg_op_gn_forward: null pointer");
    if (a->r2 && (!a->stats2 || !a->gamma2 || !a->beta2 || !a->scale2 || !a->shift2 || !a->mean2 || !a->rstd2))
        return fail("seg_op_gn_forward: null pointer (second branch)");
    if (const char* e = gn_shape_error(a->N, a->C, a->V, dtype)) return fail(std::string("seg_op_gn_forward: ") + e);
    if (a->rep < 1 || a->rep > STAT_REP) return fail("seg_op_gn_forward: rep must be 1..32");
    if ((a->mask1 || a->mask2) && a->mask_ld < a->C) return fail("seg_op_gn_forward: mask_ld must be >= C");
    if (a->path < SEG_GN_FWD_FINALIZE || a->path > SEG_GN_FWD_GROUP) return fail("seg_op_gn_forward: unknown path");
    const int esz = dtype == DT_F32 ? 4 : 2;
    GnFinArgs f1{}, f2{};
    f1.stats = a->stats1; f1.gamma = a->gamma1; f1.beta = a->beta1; f1.mask = a->mask1; f1.mask_ld = a->mask_ld;
    f1.scale = a->scale1; f1.shift = a->shift1; f1.mean = a->mean1; f1.rstd = a->rstd1;
    f1.N = a->N; f1.C = a->C; f1.V = a->V; f1.eps = a->eps; f1.rep = a->rep;
    f2 = f1;
    f2.stats = a->stats2; f2.gamma = a->gamma2; f2.beta = a->beta2; f2.mask = a->mask2;
    f2.scale = a->scale2; f2.shift = a->shift2; f2.mean = a->mean2; f2.rstd = a->rstd2;
    hipStream_t st = (hipStream_t)stream;
    if (a->path == SEG_GN_FWD_GROUP) {
        if (a->r2) return fail("seg_op_gn_forward: the one-workgroup-per-group form has no second branch");
        if (!gn_bwd_group_eligible(a->C, a->V, esz)) return fail("seg_op_gn_forward: shape not eligible for the one-workgroup-per-group form (C >= 64, <= 128 KB per sample)");
        launch_gn_fwd_group(f1, a->r1, a->res, a->out, dtype, st);
        return SEG_OK("seg_op_gn_forward");
    }
    ActArgs x{};
    x.r1 = a->r1; x.scale1 = a->scale1; x.shift1 = a->shift1;
    if (a->r2) { x.r2 = a->r2; x.scale2 = a->scale2; x.shift2 = a->shift2; }
    x.res = a->res; x.out = a->out; x.N = a->N; x.C = a->C; x.V = a->V;
    if (a->path == SEG_GN_FWD_FOLD) {
        x.fold = 1; x.fin1 = f1;
        if (a->r2) x.fin2 = f2;
    } else if (a->r2) launch_gn_finalize(f1, st, &f2);
    else launch_gn_finalize(f1, st);
    launch_gn_act(x, dtype, st);
    return SEG_OK("seg_op_gn_forward");
}

static int gn_backward_impl(const seg_gn_bwd_args* a, const GnHeadW* hw, int dtype, void* stream);
int seg_op_gn_backward(const seg_gn_bwd_args* a, int dtype, void* stream) { return gn_backward_impl(a, nullptr, dtype, stream); }
int seg_op_gn_backward_head(const seg_gn_bwd_args* a, double* head_sums, float* head_dw, float* head_db, int dtype, void* stream) {
    if (!head_sums || !head_dw || !head_db) return fail("seg_op_gn_backward_head: null pointer");
    const GnHeadW hw{head_sums, head_dw, head_db};
    return gn_backward_impl(a, &hw, dtype, stream);
}
static int gn_backward_impl(const seg_gn_bwd_args* a, const GnHeadW* hw, int dtype, void* stream) {
    if (!a || !a->r || !a->scale || !a->shift || !a->mean || !a->rstd || !a->stats || !a->gamma || !a->Q || !a->dr || !a->dgamma || !a->dbeta)
        return fail("seg_op_gn_backward: null pointer");
    if (a->r2 && (!a->scale2 || !a->shift2 || !a->mean2 || !a->rstd2 || !a->stats2 || !a->gamma2 || !a->Q2 || !a->dr2 || !a->dgamma2 || !a->dbeta2))
        return fail("seg_op_gn_backward: null pointer (second branch)");
    if (a->ndy < 0 || a->ndy > 3 || (a->ndy == 0 && !a->vdl)) return fail("seg_op_gn_backward: 1..3 stored gradient sources, or a virtual one");
    for (int i = 0; i < a->ndy; ++i)
        if (!a->dy[i]) return fail("seg_op_gn_backward: null pointer (gradient source)");
    if (a->vdl && (!a->vw || a->vK < 1 || a->vK > 16)) return fail("seg_op_gn_backward: the virtual source needs vw and vK in 1..16");
    if (const char* e = gn_shape_error(a->N, a->C, a->V, dtype)) return fail(std::string("seg_op_gn_backward: ") + e);
    if (a->rep_q < 1 || a->rep_q > STAT_REP || a->rep_s < 1 || a->rep_s > STAT_REP) return fail("seg_op_gn_backward: rep_q / rep_s must be 1..32");
    if ((a->mask || a->mask2) && a->mask_ld < a->C) return fail("seg_op_gn_backward: mask_ld must be >= C");
    if (a->path < SEG_GN_BWD_SEPARATE || a->path > SEG_GN_BWD_COOP) return fail("seg_op_gn_backward: unknown path");
    const int esz = dtype == DT_F32 ? 4 : 2;
    GnBwdArgs e{};
    for (int i = 0; i < 3; ++i) e.dy[i] = i < a->ndy ? a->dy[i] : nullptr;
    e.ndy = a->ndy; e.r = a->r; e.scale = a->scale; e.shift = a->shift; e.Q = a->Q; e.coef = a->coef; e.dr = a->dr;
    e.N = a->N; e.C = a->C; e.V = a->V;
    if (a->r2) { e.r2 = a->r2; e.scale2 = a->scale2; e.shift2 = a->shift2; e.Q2 = a->Q2; e.coef2 = a->coef2; e.dr2 = a->dr2; }
    if (a->vdl) { e.vdl = a->vdl; e.vw = a->vw; e.vK = a->vK; }
    e.rep_q = a->rep_q;
    GnBwdFinArgs f{}, f2{};
    f.Q = a->Q; f.stats = a->stats; f.gamma = a->gamma; f.mask = a->mask; f.mask_ld = a->mask_ld; f.mean = a->mean; f.rstd = a->rstd;
    f.dgamma = a->dgamma; f.dbeta = a->dbeta; f.dbias = a->dbias; f.coef = a->coef;
    f.N = a->N; f.C = a->C; f.V = a->V; f.rep_q = a->rep_q; f.rep_s = a->rep_s;
    f2 = f;
    f2.Q = a->Q2; f2.stats = a->stats2; f2.gamma = a->gamma2; f2.mask = a->mask2; f2.mean = a->mean2; f2.rstd = a->rstd2;
    f2.dgamma = a->dgamma2; f2.dbeta = a->dbeta2; f2.dbias = a->dbias2; f2.coef = a->coef2;
    hipStream_t st = (hipStream_t)stream;
    if (hw && ((a->path != SEG_GN_BWD_SEPARATE && a->path != SEG_GN_BWD_FOLD) || !gn_head_w_supported(e)))
        return fail("seg_op_gn_backward_head: reduce + apply paths only, with the virtual source of a one-class head (vK == 1), one branch, 0 or 1 stored sources, C <= 128");
    if (a->path == SEG_GN_BWD_COOP) {
        if (!gn_bwd_coop_eligible(e, esz)) return fail("seg_op_gn_backward: not eligible for the co-operative kernel (1..3 stored sources, one branch, seg_op_gn_coop_plan)");
        launch_gn_bwd_coop(e, f, dtype, st);
    } else if (a->path == SEG_GN_BWD_GROUP) {
        if (a->r2 || a->vdl || a->ndy < 1) return fail("seg_op_gn_backward: the one-workgroup-per-group form takes 1..3 stored sources and one branch");
        if (!gn_bwd_group_eligible(a->C, a->V, esz)) return fail("seg_op_gn_backward: shape not eligible for the one-workgroup-per-group form (C >= 64, <= 128 KB per sample)");
        launch_gn_bwd_group(e, f, dtype, st);
    } else {
        if (a->path == SEG_GN_BWD_SEPARATE && (!a->coef || (a->r2 && !a->coef2))) return fail("seg_op_gn_backward: null pointer (coef)");
        launch_gn_bwd_reduce(e, dtype, st, hw);
        if (a->path == SEG_GN_BWD_SEPARATE) {
            if (a->r2) launch_gn_bwd_finalize(f, st, &f2);
            else launch_gn_bwd_finalize(f, st);
            launch_gn_bwd_apply(e, dtype, st, nullptr, nullptr, hw);
        } else launch_gn_bwd_apply(e, dtype, st, &f, a->r2 ? &f2 : nullptr, hw);
    }
    return SEG_OK("seg_op_gn_backward");
}

int seg_op_gn_coop_plan(int c, long long v, int n, int esz, int* S, int* ku) {
    if (c < 8) return 0;
    return gn_bwd_coop_plan(c, v, n, esz, S, ku) ? 1 : 0;
}
int seg_op_gn_group_eligible(int c, long long v, int esz) { return gn_bwd_group_eligible(c, v, esz) ? 1 : 0; }

int seg_op_maxpool(const void* in, void* out, const void* dout, void* din, int n, int d, int h, int w, int c, int pd, int ph, int pw, int backward,
                   int dtype, void* stream) {
    if (!in || (backward ? (!dout || !din) : !out)) return fail("seg_op_maxpool: null pointer");
    if (dtype < DT_F32 || dtype > DT_BF16) return fail("seg_op_maxpool: unknown dtype");
    if (n < 1 || d < 1 || h < 1 || w < 1 || c < 8 || c % 8) return fail("seg_op_maxpool: extents must be positive and C a multiple of 8");
    if (pd < 1 || pd > 2 || ph < 1 || ph > 2 || pw < 1 || pw > 2 || d % pd || h % ph || w % pw) return fail("seg_op_maxpool: windows are 1 or 2 and divide their extents");
    PoolArgs a{};
    a.in = in; a.out = out; a.dout = dout; a.din = din; a.N = n; a.D = d; a.H = h; a.W = w; a.C = c; a.pd = pd; a.ph = ph; a.pw = pw;
    if (backward) launch_maxpool_bwd(a, dtype, (hipStream_t)stream);
    else launch_maxpool_fwd(a, dtype, (hipStream_t)stream);
    return SEG_OK("seg_op_maxpool");
}

static int cls_head_extents_ok(int n, long long v, int c) { return n >= 1 && n <= 65535 && v >= 1 && v < (1ll << 31) / CLS_K && c >= 1 && c <= 16; }
long long seg_op_cls_head_ws_bytes(int n, long long v) {
    if (!cls_head_extents_ok(n, v, 1)) return fail("seg_op_cls_head_ws_bytes: n must be 1..65535 and v in [1, 2^31 / 256)");
    return (long long)cls_head_ws_bytes(n, v);
}
long long seg_op_cls_head_ws_offset(int n, long long v, int what) {
    if (!cls_head_extents_ok(n, v, 1) || what < 0 || what > 1) return fail("seg_op_cls_head_ws_offset: bad extents, or `what` not 0 (pooled) / 1 (h)");
    return (long long)cls_head_ws_offset(n, v, what);
}
int seg_op_cls_head_forward(const void* act, const float* w1, const float* b1, const float* w2, const float* b2, float* logits, float* probs, int n,
                            long long v, int c, void* ws, int dtype, void* stream) {
    if (!act || !w1 || !b1 || !w2 || !b2 || !logits || !probs || !ws) return fail("seg_op_cls_head_forward: null pointer");
    if (dtype < DT_F32 || dtype > DT_BF16) return fail("seg_op_cls_head_forward: unknown dtype");
    if (!cls_head_extents_ok(n, v, c)) return fail("seg_op_cls_head_forward: n must be 1..65535, v in [1, 2^31 / 256), c 1..16");
    if ((uintptr_t)ws & 255) return fail("seg_op_cls_head_forward: the workspace must be 256-byte aligned");
    ClsHeadArgs a{};
    a.act = act; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.logits = logits; a.probs = probs; a.N = n; a.V = v; a.C = c; a.ws = (char*)ws;
    launch_cls_head_fwd(a, dtype, (hipStream_t)stream);
    return SEG_OK("seg_op_cls_head_forward");
}
int seg_op_cls_head_backward(const float* dlogits, const float* w1, const float* w2, float* dw1, float* db1, float* dw2, float* db2, void* dact, int n,
                             long long v, int c, int zero_grads, void* ws, int dtype, void* stream) {
    if (!dlogits || !w1 || !w2 || !dw1 || !db1 || !dw2 || !db2 || !dact || !ws) return fail("seg_op_cls_head_backward: null pointer");
    if (dtype < DT_F32 || dtype > DT_BF16) return fail("seg_op_cls_head_backward: unknown dtype");
    if (!cls_head_extents_ok(n, v, c)) return fail("seg_op_cls_head_backward: n must be 1..65535, v in [1, 2^31 / 256), c 1..16");
    if ((uintptr_t)ws & 255) return fail("seg_op_cls_head_backward: the workspace must be 256-byte aligned");
    ClsHeadArgs a{};
    a.dlogits = dlogits; a.w1 = w1; a.w2 = w2; a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2; a.dact = dact; a.accumulate = zero_grads ? 0 : 1;
    a.N = n; a.V = v; a.C = c; a.ws = (char*)ws;
    launch_cls_head_bwd(a, dtype, (hipStream_t)stream);
    return SEG_OK("seg_op_cls_head_backward");
}

static const char* gradcam_shape_error(int n, int c, int id, int ih, int iw, int od, int oh, int ow) {
    if (n < 1 || n > 65535) return "n must be 1..65535";
    if (c != 16 && c != 32 && c != 64 && c != 128 && c != 256) return "c must be 16, 32, 64, 128 or 256";
    if (id < 1 || ih < 1 || iw < 1 || od < 1 || oh < 1 || ow < 1) return "every extent must be >= 1";
    if ((long long)id * ih * iw >= (1ll << 31) / c || (long long)od * oh * ow >= (1ll << 31)) return "id * ih * iw * c and od * oh * ow must stay below 2^31";
    return nullptr;
}
long long seg_op_gradcam_ws_bytes(int n, int c, int id, int ih, int iw, int od, int oh, int ow) {
    if (const char* err = gradcam_shape_error(n, c, id, ih, iw, od, oh, ow)) return fail(std::string("seg_op_gradcam_ws_bytes: ") + err);
    return (long long)gradcam_ws_bytes(n, c, (long long)id * ih * iw, (long long)od * oh * ow);
}
int seg_op_gradcam(const void* act, const void* grad, int dtype, int n, int c, int id, int ih, int iw, int od, int oh, int ow, int ndim, float inv_loss_scale,
                   float weight, int accumulate, int finalize, void* ws, float* out, void* stream) {
    if (!act || !grad || !ws || !out) return fail("seg_op_gradcam: null pointer");
    if (dtype < DT_F32 || dtype > DT_BF16) return fail("seg_op_gradcam: unknown dtype");
    if (ndim != 2 && ndim != 3) return fail("seg_op_gradcam: ndim must be 2 or 3");
    if (ndim == 2 && (id != 1 || od != 1)) return fail("seg_op_gradcam: ndim 2 takes id = od = 1");
    if (const char* err = gradcam_shape_error(n, c, id, ih, iw, od, oh, ow)) return fail(std::string("seg_op_gradcam: ") + err);
    if (!(inv_loss_scale > 0.f) || !std::isfinite(inv_loss_scale) || !(weight > 0.f) || !std::isfinite(weight))
        return fail("seg_op_gradcam: inv_loss_scale and weight must be positive and finite");
    if (((uintptr_t)act | (uintptr_t)grad) & 31) return fail("seg_op_gradcam: act and grad must be 32-byte aligned");
    if ((uintptr_t)ws & 255) return fail("seg_op_gradcam: the workspace must be 256-byte aligned");
    GradCamArgs a{};
    a.act = act; a.grad[0] = grad; a.ngrad = 1; a.out = out; a.N = n; a.C = c; a.ID = id; a.IH = ih; a.IW = iw; a.OD = od; a.OH = oh; a.OW = ow;
    a.inv_scale = inv_loss_scale; a.weight = weight; a.accumulate = accumulate ? 1 : 0; a.finalize = finalize ? 1 : 0; a.ws = (char*)ws;
    launch_gradcam_layer(a, dtype, (hipStream_t)stream);
    return SEG_OK("seg_op_gradcam");
}

int seg_op_pool3(const float* x, float* out, int planes, int d, int h, int w, int nd, int is_min, void* stream) {
    if (!x || !out || (nd != 2 && nd != 3)) return fail("seg_op_pool3: bad arguments");
    launch_pool3(x, out, planes, d, h, w, nd, is_min, (hipStream_t)stream);
    return SEG_OK("seg_op_pool3");
}
int seg_op_skel_iter(const float* x, float* e_out, float* x_out, int planes, int d, int h, int w, int nd, void* stream) {
    if (!x || !e_out || !x_out || (nd != 2 && nd != 3)) return fail("seg_op_skel_iter: bad arguments");
    launch_skel_iter(x, e_out, x_out, planes, d, h, w, nd, (hipStream_t)stream);
    return SEG_OK("seg_op_skel_iter");
}
int seg_op_skel_iter_bwd(const float* g, const float* x, const float* e, float* dx, float* de_scratch, int planes, int d, int h, int w, int nd,
                         void* stream) {
    if (!g || !x || !e || !dx || !de_scratch || (nd != 2 && nd != 3)) return fail("seg_op_skel_iter_bwd: bad arguments");
    launch_skel_iter_bwd(g, x, e, dx, de_scratch, planes, d, h, w, nd, (hipStream_t)stream);
    return SEG_OK("seg_op_skel_iter_bwd");
}
int seg_op_skel_update(const float* x, const float* e, float* out, int planes, int d, int h, int w, int nd, void* stream) {
    if (!x || !e || !out || (nd != 2 && nd != 3)) return fail("seg_op_skel_update: bad arguments");
    launch_skel_update(x, e, out, planes, d, h, w, nd, (hipStream_t)stream);
    return SEG_OK("seg_op_skel_update");
}
int seg_op_skel_update_bwd(const float* g, const float* x, const float* e, float* dx, float* de, int planes, int d, int h, int w, int nd,
                           void* stream) {
    if (!g || !x || !e || !dx || !de || (nd != 2 && nd != 3)) return fail("seg_op_skel_update_bwd: bad arguments");
    launch_skel_update_bwd(g, x, e, dx, de, planes, d, h, w, nd, (hipStream_t)stream);
    return SEG_OK("seg_op_skel_update_bwd");
}
int seg_op_pool3_bwd(const float* src, const float* dout, float* din, int planes, int d, int h, int w, int nd, int is_min, void* stream) {
    if (!src || !dout || !din || (nd != 2 && nd != 3)) return fail("seg_op_pool3_bwd: bad arguments");
    launch_pool3_bwd(src, dout, din, planes, d, h, w, nd, is_min, (hipStream_t)stream);
    return SEG_OK("seg_op_pool3_bwd");
}
long long seg_op_plane_dot_scratch_bytes(int planes, long long v) { return (long long)plane_dot_scratch_bytes(planes, v); }
int seg_op_plane_dot(const float* a, const float* b, double* out2, double* scratch, int planes, long long v, void* stream) {
    if (!a || !b || !out2 || !scratch) return fail("seg_op_plane_dot: null pointer");
    launch_plane_dot(a, b, out2, scratch, planes, v, (hipStream_t)stream);
    return SEG_OK("seg_op_plane_dot");
}
int seg_op_plane_axpb(const float* in, const float* a, const float* b, float* out, int planes, long long v, int accumulate, void* stream) {
    if (!in || !a || !b || !out) return fail("seg_op_plane_axpb: null pointer");
    launch_plane_axpb(in, a, b, out, planes, v, accumulate, (hipStream_t)stream);
    return SEG_OK("seg_op_plane_axpb");
}

long long seg_cldice_ws_bytes(int n, int d, int h, int w, int nd, int width) {
    if (n < 1 || h < 1 || w < 1 || width < 0 || (nd != 2 && nd != 3)) return -1;
    return (long long)cldice_binary_ws_bytes(n, (long long)(nd == 3 ? d : 1) * h * w, width);
}
int seg_cldice_target(const void* target, int label_type, int n, int d, int h, int w, int nd, int width, void* ws, void* stream) {
    if (!target || !ws) return fail("seg_cldice_target: null pointer");
    if (n < 1 || h < 1 || w < 1 || width < 0 || (nd != 2 && nd != 3)) return fail("seg_cldice_target: bad extents");
    launch_cldice_target(target, label_type, n, nd == 3 ? d : 1, h, w, nd, width, ws, (hipStream_t)stream);
    return SEG_OK("seg_cldice_target");
}
int seg_cldice_binary(const float* probs, const void* target, int label_type, int n, int d, int h, int w, int nd, int width,
                      float grad_scale, void* ws, float* out1, float* dlogits, int target_ready, void* stream) {
    if (!probs || !target || !ws || !out1) return fail("seg_cldice_binary: null pointer");
    if (n < 1 || h < 1 || w < 1 || width < 0 || (nd != 2 && nd != 3)) return fail("seg_cldice_binary: bad extents");
    launch_cldice_binary(probs, target, label_type, n, nd == 3 ? d : 1, h, w, nd, width, grad_scale, ws, out1, dlogits, target_ready,
                         (hipStream_t)stream);
    return SEG_OK("seg_cldice_binary");
}

}  // extern "C"

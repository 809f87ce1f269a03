"""float64 numpy restatement of the seg_augment2d contract (include/segengine.h): flip, blur, warp, tone - gather indices and explicit loops over taps.
It shares no code with the product, and it is NOT albumentations / cv2 (neither can run here; the contract is this project's own definition).

apply(x, p, ...) takes ONE sample: x (C, H, W), the 64-double parameter block p, an optional label (H, W).  It returns (image float64 (C, H, W), label
or None, margin): margin is the smallest distance of any floor decision of the warp (sy, sx, sy + 0.5, sx + 0.5) from an integer - the room a
last-bit difference of a coordinate would need to change a tap or a label pixel.  When every coordinate is computed EXACTLY whatever the order of
the operations (all six entries of M are multiples of 2^-20 below 2^20 and the image is smaller than 4096 x 4096: every product and sum then fits a
double's 53 bits), a decision that sits on an integer is not at risk and the margin is inf; the same without a warp."""
import numpy as np

NEAREST, CONSTANT, MIRROR = 0, 1, 4


def fold_mirror(i, n):
    """d c b | a b c d: period 2(n - 1), 0 for n == 1; i any int64 array"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    m = np.mod(i, period)
    return np.where(m > n - 1, period - m, m)


def border_index(i, n, mode):
    """(index into the axis, outside mask) for integer positions i"""
    i = np.asarray(i, dtype=np.int64)
    outside = (i < 0) | (i > n - 1)
    if mode == MIRROR:
        return fold_mirror(i, n), np.zeros_like(outside)
    clamped = np.clip(i, 0, n - 1)
    return clamped, (outside if mode == CONSTANT else np.zeros_like(outside))


def coordinates_exact(m, h, w):
    scaled = m * 2.0 ** 20
    return bool(np.all(scaled == np.rint(scaled)) and np.all(np.abs(m) < 2.0 ** 20) and h < 4096 and w < 4096)


def apply(x, p, label=None, border=MIRROR, cval=0.0, label_cval=0):
    x = np.asarray(x, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    c, h, w = x.shape
    flips, warp, blur, k = int(p[6]), p[7] != 0, int(p[8]), int(p[9])
    # 1. flip
    ys = np.arange(h)[::-1] if flips & 2 else np.arange(h)
    xs = np.arange(w)[::-1] if flips & 1 else np.arange(w)
    f = x[:, ys][:, :, xs]
    lab = None if label is None else np.asarray(label)[ys][:, xs]
    # 2. blur (image only)
    if blur == 1:
        wts = np.append(p[16:64], p[15])[:k * k].reshape(k, k)          # (the 49th weight of a 7 x 7 kernel lives in slot 15)
        g = np.zeros_like(f)
        for ky in range(k):
            iy = fold_mirror(np.arange(h) + ky - k // 2, h)
            for kx in range(k):
                ix = fold_mirror(np.arange(w) + kx - k // 2, w)
                g += wts[ky, kx] * f[:, iy][:, :, ix]
    elif blur == 2:
        shifted = []
        for dy in (-1, 0, 1):
            iy = np.clip(np.arange(h) + dy, 0, h - 1)
            for dx in (-1, 0, 1):
                ix = np.clip(np.arange(w) + dx, 0, w - 1)
                shifted.append(f[:, iy][:, :, ix])
        g = np.sort(np.stack(shifted), axis=0)[4]
    else:
        g = f
    # 3. warp
    margin = np.inf
    if warp:
        m = p[0:6].reshape(2, 3)
        yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        sy = (yy * m[0, 0] + xx * m[0, 1]) + m[0, 2]
        sx = (yy * m[1, 0] + xx * m[1, 1]) + m[1, 2]
        if not coordinates_exact(m, h, w):
            margin = min(float(np.min(np.abs(v - np.rint(v)))) for v in (sy, sx, sy + 0.5, sx + 0.5))
        fy, fx = np.floor(sy), np.floor(sx)
        wy, wx = sy - fy, sx - fx
        taps = {}
        for r in (0, 1):
            iy, oy = border_index(fy.astype(np.int64) + r, h, border)
            for q in (0, 1):
                ix, ox = border_index(fx.astype(np.int64) + q, w, border)
                v = g[:, iy, ix]
                taps[r, q] = np.where((oy | ox)[None], float(cval), v)
        top = (1 - wx) * taps[0, 0] + wx * taps[0, 1]
        bot = (1 - wx) * taps[1, 0] + wx * taps[1, 1]
        out = (1 - wy) * top + wy * bot
        if lab is not None:
            iy, oy = border_index(np.floor(sy + 0.5).astype(np.int64), h, border)
            ix, ox = border_index(np.floor(sx + 0.5).astype(np.int64), w, border)
            lab = np.where(oy | ox, np.asarray(label_cval).astype(lab.dtype), lab[iy, ix])
    else:
        out = g
    # 4. tone (image only)
    if not (p[10] == 1.0 and p[11] == 0.0):
        out = p[10] * out + p[11]
    if p[12] != 0:
        out = np.clip(out, p[13], p[14])
    return out, lab, margin

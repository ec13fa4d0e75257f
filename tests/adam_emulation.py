"""MXNet 1.2 `Adam.update` / `adam_update`, restated in numpy from its definition (the operator is not part of the reference
checkout): the arithmetic contract of deepim_adam_update / deepim_adam_update_multi (include/deepim_hip.h).

    g'   = rescale_grad * g + wd * w
    g'   = clamp(g', +-clip_gradient)          if clip_gradient > 0 (0 / None: no clip) — AFTER the weight-decay term
    m    = beta1 * m + (1 - beta1) * g'
    v    = beta2 * v + (1 - beta2) * g' * g'
    w    = w - lr_t * m / (sqrt(v) + epsilon)  epsilon outside the bias correction, unlike torch.optim.Adam
    lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), evaluated in double, rounded to float once; t counts the updates applied, this
           one included. A skipped step (overflowed gradients in the loss-scaled modes) moves nothing and does not advance t.

dtype = float64 is the reference the GPU tests compare against (fed the same float32 arrays); dtype = float32 runs the same
operations in the kernel's order and precision (the kernels are built without FMA contraction)."""
import numpy as np

BETA1, BETA2, EPSILON = 0.9, 0.999, 1e-8


def lr_t(lr, t, beta1=BETA1, beta2=BETA2, as_float=True):
    """The bias-corrected learning rate of update number t (>= 1): the float the kernel reads, or (as_float = False) the double."""
    v = float(lr) * np.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t)
    return np.float32(v) if as_float else v


def adam_update(w, m, v, g, lr, t, wd=0.0, beta1=BETA1, beta2=BETA2, epsilon=EPSILON, rescale=1.0, clip=None, skip=False,
                dtype=np.float64, float_lr_t=True):
    """One update. t = the number of updates applied BEFORE this one. -> (w, m, v, t, g') after it, arrays in `dtype`; skip = True
    (the overflow word is set) returns the inputs and the same t. float_lr_t = False keeps lr_t a double: the formula itself, without the
    one rounding that belongs to the kernel's contract."""
    f = np.dtype(dtype).type
    w, m, v, g = (np.asarray(a).astype(dtype) for a in (w, m, v, g))
    if skip:
        return w, m, v, t, None
    t = t + 1
    # the scalars: exact in float64; in float32 as the kernel holds them (beta and 1 - beta rounded separately from the doubles)
    b1, omb1, b2, omb2, eps, rs, wdf = (f(x) for x in (beta1, 1.0 - beta1, beta2, 1.0 - beta2, epsilon, rescale, wd))
    gp = g * rs + wdf * w
    if clip is not None and clip > 0:
        cl = f(clip)
        gp = np.minimum(np.maximum(gp, -cl), cl)
    m = b1 * m + omb1 * gp
    v = b2 * v + omb2 * gp * gp
    w = w - f(lr_t(lr, t, beta1, beta2, float_lr_t)) * m / (np.sqrt(v) + eps)
    return w, m, v, t, gp


def bounds(w_ref, m_old, v_ref, gp_ref, lrt, beta1=BETA1):
    """The error bars of a float32 evaluation against the float64 one on the same float32 inputs: a handful of fp32 roundings (6e-8
    each) on the terms of every sum (m_old: the first moment BEFORE the update, the term beta1*m of its sum); the second term on w
    carries the moment error through m / sqrt(v) <= (1-beta1)/sqrt(1-beta2) and a last-bit difference in the float lr_t.
    -> (bound on |dw|, on |dm|, on |dv|)"""
    return (1e-6 * np.abs(w_ref) + 2e-5 * float(lrt),
            1e-6 * (beta1 * np.abs(np.asarray(m_old, np.float64)) + (1.0 - beta1) * np.abs(gp_ref)),
            1e-6 * v_ref)


def check(got_w, got_m, got_v, ref, m_old, lrt, tag=""):
    """Assert (w, m, v) within bounds() of ref = the result of adam_update(..., dtype=float64) on the same float32 inputs."""
    w_ref, m_ref, v_ref, _t, gp = ref
    bw, bm, bv = bounds(w_ref, m_old, v_ref, gp, lrt)
    for name, got, want, bar in (("mean", got_m, m_ref, bm), ("var", got_v, v_ref, bv), ("w", got_w, w_ref, bw)):
        err = np.abs(np.asarray(got, np.float64) - want)
        bad = err > bar
        assert not bad.any(), "%s %s: %d of %d outside the bound, worst |d| = %.3g at bound %.3g" % (
            tag, name, int(bad.sum()), bad.size, float(err[bad].max()), float(bar[bad][np.argmax(err[bad])]))


# ---- the synthetic parameter table of the kernel tests (tests/test_gpu_adam.py; its float32 behaviour is checked on the CPU in
# tests/test_adam_host.py): 70 rows, so the kernel's 64-rows-per-ballot row lookup runs a second round
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4098]
TAP_MAJOR = {7: (3, 8, 9), 30: (5, 16, 25), 66: (8, 8, 49)}      # row -> (Cout, Cin, taps); 8*8*49 = 3136: more than one block
ROWS = 70


def table_rows():
    """-> [(n, wd, (Cout, Cin, taps) or None)] per row."""
    out = []
    for i in range(ROWS):
        tm = TAP_MAJOR.get(i)
        n = tm[0] * tm[1] * tm[2] if tm else SIZES[i % len(SIZES)]
        out.append((n, 5e-4 if i % 2 else 0.0, tm))
    return out


def table_weights(rng):
    return [rng.standard_normal(n).astype(np.float32) for n, _wd, _tm in table_rows()]


def table_gradients(rng):
    """Fresh gradients in the parameters' natural layout: random signs, magnitudes in [0.1, 2) (so rescale*g never cancels against
    wd*w, which would put the whole rounding of the larger terms on a small g'), and about one in eight exactly zero. Every fourth
    row of size >= 4 has its first four gradients zero: with zero moments and wd = 0 those weights must keep their bits."""
    out = []
    for i, (n, _wd, _tm) in enumerate(table_rows()):
        g = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.1, 2.0, n)).astype(np.float32)
        g[rng.random(n) < 0.125] = 0.0
        if i % 4 == 0 and n >= 4:
            g[:4] = 0.0
        out.append(g)
    return out


def to_tap_major(g, cout, cin, taps):
    """natural (Cout, Cin, taps) -> the (Cout, taps, Cin) layout of deepim_conv2d_wgrad_tm."""
    return np.ascontiguousarray(g.reshape(cout, cin, taps).transpose(0, 2, 1)).ravel()

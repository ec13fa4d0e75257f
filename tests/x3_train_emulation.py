"""Emulation of the split-fp16 training iteration (TRAIN.X3_CONV), composed from oracle primitives. TEST INFRASTRUCTURE ONLY.

Arithmetic contract. split(v, s): hi = f16(clamp(v·s, ±60000)), lo = f16(clamp(v·s) − hi); a product of two
pairs is hi·hi + hi·lo + lo·hi with fp32 accumulation. S = the gradient scale; activations are stored at scale 16:
  forward   y_-1 = split(net_input, 16), y_l = split(lrelu(conv(y_l-1, split(w_l, s_w)) + b_l), 16); FC head, losses, decoder and
            heads fp32 on the pair values
  e_l       S·(fc6 data gradient + d_dec61) at conv6_1; d_l [+ S·skip_l] below (skip: decoder gradient of conv5_1 / conv4_1)
  dz_l      split(lrelu'(y_l)·e_l, 1)
  db_l      Σ dz_l / S;  dW_l = Σ_pix dz_l ⊗ im2col(y_l-1) / (16·S)
  d_l-1     split(conv_transpose(dz_l, split(w_l, s_w)) / s_w, 1)                       (not for flow_conv1)
  the two layers on the fp32 kernels: dW of flow_conv1 = Σ_pix (dz / S) ⊗ im2col(net_input); d of conv2 from the unsplit weights
`train_iteration` works on the VALUES of the pairs (`pair_value`): the three-term product of two pairs differs from the product
of their values by the lo·lo term, 2^-22 relative, below the fp32 accumulation it is added into — the GPU tests hold the kernels
to 1e-5 / 2e-4 bars against it, not bit for bit. `matmul3` is the three-term product itself, for the accuracy window of the scale.
With `split` the identity and S = 1 `train_iteration` is oracle.pipeline.train_iteration exactly (tests/test_x3_train_host.py).
`acts` (optional): the encoder outputs to differentiate at (the GPU's own pair values) instead of the emulated forward."""
import numpy as np

from oracle import heads as oheads
from oracle import net as onet
from oracle import pipeline as opipe
from oracle import se3 as ose3
from oracle import zoom as ozoom

f32 = np.float32
SLOPE = 0.1
ENCODER = opipe.ENCODER
ACT_SCALE = 16.0


def split(v, scale):
    """x3_split -> (hi, lo) as float32 arrays holding fp16 values."""
    x = np.clip((np.asarray(v, f32) * f32(scale)).astype(f32), f32(-60000.0), f32(60000.0)).astype(f32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(f32)).astype(np.float16)
    return hi.astype(f32), lo.astype(f32)


def clamps(v, scale):
    """Whether split(v, scale) clamps or meets a non-finite value (what raises the overflow word)."""
    return bool(np.any(~(np.abs((np.asarray(v, f32) * f32(scale)).astype(f32)) <= f32(60000.0))))


def pair_value(v, scale):
    """The real value the pair split(v, scale) carries: (hi + lo) / scale in fp32 (scale a power of two)."""
    hi, lo = split(v, scale)
    return ((hi + lo).astype(f32) * f32(1.0 / scale)).astype(f32)


def weight_scale(w):
    """The power of two the host picks for a weight tensor at bind time: max |w|·s in [768, 1536]."""
    m = float(np.abs(w).max())
    return 2.0 ** int(np.floor(np.log2(1536.0 / m))) if m > 0 else 1.0


def identity(v, scale=1.0):
    return np.asarray(v, f32)


def matmul3(a, b, s_a, s_b):
    """(M,K) @ (K,N) in x3 arithmetic: operands split at s_a / s_b, three fp16 products per pair (exact in fp32), fp32 accumulation
    over 16-wide k-steps (one 32x32x16 MFMA each), the result back in real units."""
    ah, al = split(a, s_a)
    bh, bl = split(b, s_b)
    acc = np.zeros((a.shape[0], b.shape[1]), f32)
    for k0 in range(0, a.shape[1], 16):
        sl = slice(k0, k0 + 16)
        part = ah[:, sl].astype(np.float64) @ bh[sl].astype(np.float64)
        part += ah[:, sl].astype(np.float64) @ bl[sl].astype(np.float64)
        part += al[:, sl].astype(np.float64) @ bh[sl].astype(np.float64)
        acc = (acc + part.astype(f32)).astype(f32)
    return (acc * f32(1.0 / (s_a * s_b))).astype(f32)


def im2col3x3(x):
    """(C,H,W) -> (H*W, 9*C), taps outermost (ky, kx, c): the 3x3 stride-1 pad-1 patch of every pixel."""
    C, H, W = x.shape
    xp = np.zeros((C, H + 2, W + 2), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    cols = [xp[:, ky:ky + H, kx:kx + W].reshape(C, H * W).T for ky in range(3) for kx in range(3)]
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def encoder(params, x, split_value=pair_value):
    acts = {}
    x = split_value(x, ACT_SCALE)
    for name, s, p in ENCODER:
        w = params[name + "_weight"]
        x = split_value(onet.conv2d(x, split_value(w, weight_scale(w)), params[name + "_bias"], s, p, SLOPE), ACT_SCALE)
        acts[name] = x
    return acts


def train_iteration(params, data, label, K, pixel_means_rev, T_means, T_stds, rot_coord="CAMERA", lw_pm=0.1, num_3d_sample=3000,
                    normalize_3d=0.1, loss_type="L1", sigma=1.0, pred_flow=False, pred_mask=False, lw_flow=0.25, lw_mask=0.03,
                    normalize_flow=20.0, split_value=pair_value, S=1.0, acts=None):
    """-> (loss_sum, grads keyed like params, forward dict with the scaled dz of every encoder layer under "dz_<name>" and
    "overflow": whether a split of the backward clamped)."""
    S = f32(S)
    x, zf = ozoom.net_input(data["image_observed"], data["image_rendered"], data["mask_observed"], data["mask_rendered"],
                            data["src_pose"], K, pixel_means_rev, data.get("depth_observed"), data.get("depth_rendered"),
                            mask_gt_observed=label["mask_gt_observed"])
    if acts is None:
        acts = encoder(params, x, split_value)
    B, _, H, W = x.shape
    P = params
    feat = acts["conv6_1"].reshape(B, -1)
    fc6 = onet.fc(feat, P["fc6_weight"], P["fc6_bias"], SLOPE)
    fc7 = onet.fc(fc6, P["fc7_weight"], P["fc7_bias"], SLOPE)
    rot = onet.fc(fc7, P["rot_weight"], P["rot_bias"], 1.0)
    ztr = onet.fc(fc7, P["trans_weight"], P["trans_bias"], 1.0)
    rot_norm = oheads.l2_normalize(rot)
    trans_est = ozoom.zoom_trans(zf, ztr, b_inv_zoom=True)
    pts = ose3.transform3d_forward(label["point_cloud_model"], rot_norm, trans_est, data["src_pose"], T_means, T_stds, rot_coord)
    loss, loss_sum, d_pts = oheads.point_matching_loss(pts, label["point_cloud_observed"], label["point_cloud_weights"],
                                                       normalize_3d, loss_type, sigma, lw_pm / num_3d_sample)
    fwd = dict(acts, net_input=x, zoom_factor=zf, fc6=fc6, fc7=fc7, rot_norm=rot_norm, trans_est=trans_est, pm_loss=loss)
    g, d_skip, d_dec61 = {}, {}, None
    if pred_flow or pred_mask:
        dec = opipe.decoder(P, acts)
        fwd.update(dec)
        C3, C2 = dec["Concat3"], dec["Concat2"]
        dC3 = np.zeros_like(C3)
        if pred_flow:
            low = onet.conv2d(C3, P["Convolution3_weight"], P["Convolution3_bias"], 1, 1, 1.0)
            est = onet.upsample16_crop(low, P["upsampling_weight"], H, W, (8, 8), 1.0)
            zflow, zfw = ozoom.zoom_flow(zf, label["flow"], label["flow_weights"], b_inv_zoom=False)
            fl, fl_sum, d_est = oheads.flow_loss(est, zflow, zfw, normalize_flow, lw_flow / (480 * 640))
            d_low = onet.upsample16_crop_backward(d_est, P["upsampling_weight"], 30, 40, (8, 8), 1.0)
            dx, g["Convolution3_weight"], g["Convolution3_bias"] = onet.conv2d_backward(C3, P["Convolution3_weight"], d_low, 1, 1)
            dC3 += dx
            g["upsampling_weight"] = np.zeros_like(P["upsampling_weight"])
            fwd.update(flow_loss_sum=fl_sum)
        if pred_mask:
            low = onet.conv2d(C3, P["mask_conv3_weight"], P["mask_conv3_bias"], 1, 1, 1.0)
            logits = onet.upsample16_crop(low, P["mask_upsampling_weight"], H, W, (8, 8), 1.0)
            zgt = ozoom.zoom_mask(data["mask_observed"], label["mask_gt_observed"], data["mask_rendered"], data["src_pose"], K)[1]
            prob, d_logits = oheads.mask_logistic(logits, zgt, lw_mask / (H * W))
            d_low = onet.upsample16_crop_backward(d_logits, P["mask_upsampling_weight"], 30, 40, (8, 8), 1.0)
            dx, g["mask_conv3_weight"], g["mask_conv3_bias"] = onet.conv2d_backward(C3, P["mask_conv3_weight"], d_low, 1, 1)
            dC3 += dx
            g["mask_upsampling_weight"] = np.zeros_like(P["mask_upsampling_weight"])
            fwd.update(mask_prob=prob)
        d_skip["conv4_1"] = np.ascontiguousarray(dC3[:, :512])
        d_d4 = onet.lrelu_backward(dC3[:, 512:768], C3[:, 512:768], SLOPE)
        dC2, g["deconv4_weight"], g["deconv4_bias"] = onet.deconv4x4s2_crop_backward(C2, P["deconv4_weight"], d_d4)
        d_f5, g["upsample_flow5to4_weight"], g["upsample_flow5to4_bias"] = onet.deconv4x4s2_crop_backward(
            dec["flow5"], P["upsample_flow5to4_weight"], dC3[:, 768:770])
        dx, g["Convolution2_weight"], g["Convolution2_bias"] = onet.conv2d_backward(C2, P["Convolution2_weight"], d_f5, 1, 1)
        dC2 = (dC2 + dx).astype(f32)
        d_skip["conv5_1"] = np.ascontiguousarray(dC2[:, :512])
        d_d5 = onet.lrelu_backward(dC2[:, 512:1024], C2[:, 512:1024], SLOPE)
        d_dec61, g["deconv5_weight"], g["deconv5_bias"] = onet.deconv4x4s2_crop_backward(acts["conv6_1"], P["deconv5_weight"], d_d5)
        d_f6, g["upsample_flow6to5_weight"], g["upsample_flow6to5_bias"] = onet.deconv4x4s2_crop_backward(
            dec["flow6"], P["upsample_flow6to5_weight"], dC2[:, 1024:1026])
        dx, g["Convolution1_weight"], g["Convolution1_bias"] = onet.conv2d_backward(acts["conv6_1"], P["Convolution1_weight"], d_f6, 1, 1)
        d_dec61 = (d_dec61 + dx).astype(f32)
    d_rot_norm, d_trans_est = ose3.transform3d_backward(d_pts, label["point_cloud_model"], rot_norm, trans_est, data["src_pose"],
                                                        T_means, T_stds, rot_coord)
    d_ztr = ozoom.zoom_trans_backward(zf, d_trans_est, b_inv_zoom=True, b_zoom_grad=False)
    d_rot = oheads.l2_normalize_backward(d_rot_norm, rot)
    dx_r, g["rot_weight"], g["rot_bias"] = onet.fc_backward(fc7, P["rot_weight"], d_rot)
    dx_t, g["trans_weight"], g["trans_bias"] = onet.fc_backward(fc7, P["trans_weight"], d_ztr)
    d = onet.lrelu_backward((dx_r + dx_t).astype(f32), fc7, SLOPE)
    d, g["fc7_weight"], g["fc7_bias"] = onet.fc_backward(fc6, P["fc7_weight"], d)
    d = onet.lrelu_backward(d, fc6, SLOPE)
    d, g["fc6_weight"], g["fc6_bias"] = onet.fc_backward(feat, P["fc6_weight"], d)
    d = d.reshape(acts["conv6_1"].shape)
    if d_dec61 is not None:
        d = (d + d_dec61).astype(f32)
    e = (S * d).astype(f32)                                             # e at conv6_1: S·(fc6 data gradient + d_dec61)
    overflow = False
    inv_s = f32(1.0) / S
    for li in range(len(ENCODER) - 1, -1, -1):
        name, s, p = ENCODER[li]
        if name in d_skip:
            e = (e + S * d_skip[name]).astype(f32)
        t = onet.lrelu_backward(e, acts[name], SLOPE)
        overflow |= clamps(t, 1.0)
        dz = split_value(t, 1.0)
        fwd["dz_" + name] = dz
        w = P[name + "_weight"]
        if li == 0:      # the fp32 weight gradient from the unsplit net input and dz in real units
            # (S is a power of two: Σ (dz / S) = (Σ dz) / S, the bias gradient of the contract)
            _, g[name + "_weight"], g[name + "_bias"] = onet.conv2d_backward(x, w, (dz * inv_s).astype(f32), s, p, need_dx=False)
            break
        # conv2's data gradient runs on the fp32 kernel from the unsplit weights
        wq = w if li == 1 else split_value(w, weight_scale(w))
        dx, dw, db = onet.conv2d_backward(acts[ENCODER[li - 1][0]], wq, dz, s, p, need_dx=True)
        g[name + "_weight"], g[name + "_bias"] = (dw * inv_s).astype(f32), (db * inv_s).astype(f32)
        overflow |= clamps(dx, 1.0)
        e = split_value(dx, 1.0)
    fwd["overflow"] = overflow
    return loss_sum, g, fwd

"""Numpy restatement of the fp16 Winograd F(2x2,3x3) arithmetic contract of csrc/wino_f16.hip (TEST INFRASTRUCTURE), vectorised over
tiles. Layer: Convolution 3x3 stride 1 pad 1 + bias + LeakyReLU on fp16 activations and weights.

  weights   U = q(G q(w) G^T), the products in `wdtype` (float32: the pack kernel's adds in the pack kernel's order, bit for bit)
  input     T = B^T d, V = T B, every entry one add or subtract rounded by q — two fp16 roundings
  product   sixteen sums over the input channels in `acc` (float64: the reference the GPU tests compare against; float32: a matmul
            in the kernel's precision, another order)
  output    Y = A^T M A in `acc` (the kernel's order of adds), + bias, LeakyReLU, q

q = identity and float64 everywhere turns this into the exact Winograd identity (tests/test_fp16_wino_host.py)."""
import numpy as np

from oracle import net as onet
from oracle import pipeline as opipe

q16 = opipe.q16


def identity(x):
    return x


def transform_weights(w, q=q16, wdtype=np.float32):
    """(Cout,Cin,3,3) -> U (Cout,Cin,4,4), U[..., i, nu]: position p = 4 i + nu. The adds in the order csrc/wino_f16.hip states."""
    g = np.asarray(q(w), wdtype)
    half = wdtype(0.5)
    s = g[:, :, 0, :] + g[:, :, 2, :]
    t = np.stack([g[:, :, 0, :], (s + g[:, :, 1, :]) * half, (s - g[:, :, 1, :]) * half, g[:, :, 2, :]], axis=2)     # (Cout,Cin,4,3)
    s = t[..., 0] + t[..., 2]
    u = np.stack([t[..., 0], (s + t[..., 1]) * half, (s - t[..., 1]) * half, t[..., 2]], axis=3)                     # (Cout,Cin,4,4)
    return np.asarray(q(u), wdtype)


def transform_input(x, q=q16):
    """(B,Cin,H,W) -> V[i][nu] of shape (B,Cin,TY,TX); out-of-image patch pixels are zeros."""
    B, C, H, W = x.shape
    TY, TX = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((B, C, 2 * TY + 2, 2 * TX + 2), np.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = q(x)
    d = [[xp[:, :, i:i + 2 * TY:2, j:j + 2 * TX:2] for j in range(4)] for i in range(4)]
    T = [[q(d[0][j] - d[2][j]) for j in range(4)], [q(d[1][j] + d[2][j]) for j in range(4)],
         [q(d[2][j] - d[1][j]) for j in range(4)], [q(d[1][j] - d[3][j]) for j in range(4)]]
    return [[q(T[i][0] - T[i][2]), q(T[i][1] + T[i][2]), q(T[i][2] - T[i][1]), q(T[i][1] - T[i][3])] for i in range(4)]


def conv_wino(x, w, b, slope, q=q16, acc=np.float64, wdtype=np.float32, pre_round=False):
    """The layer under the contract: (B,Cin,H,W), (Cout,Cin,3,3), (Cout,) -> (B,Cout,H,W). pre_round: return the value before the
    output rounding (in `acc`)."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    TY, TX = (H + 1) // 2, (W + 1) // 2
    U = transform_weights(w, q, wdtype).astype(acc)
    V = transform_input(np.asarray(x, np.float64), q)
    M = [[None] * 4 for _ in range(4)]
    for i in range(4):
        for nu in range(4):
            v = np.asarray(V[i][nu], acc).reshape(B, Cin, TY * TX)
            M[i][nu] = np.matmul(U[:, :, i, nu], v)                       # (B,Cout,TY*TX)
    P = [[(M[0][nu] + M[1][nu]) + M[2][nu] for nu in range(4)], [(M[1][nu] - M[2][nu]) - M[3][nu] for nu in range(4)]]
    out = np.zeros((B, Cout, 2 * TY, 2 * TX), acc)
    bias = np.asarray(b, np.float32).astype(acc).reshape(1, Cout, 1)
    sl = acc(np.float32(slope))
    for a in range(2):
        Y = [(P[a][0] + P[a][1]) + P[a][2], (P[a][1] - P[a][2]) - P[a][3]]
        for e in range(2):
            y = Y[e] + bias
            y = np.where(y > 0, y, y * sl)
            out[:, :, a::2, e::2] = y.reshape(B, Cout, TY, TX)
    out = out[:, :, :H, :W]
    return out if pre_round else q(out)


def encoder(params, x, wino_layers, q=q16, acc=np.float64):
    """The fp16 encoder (oracle.pipeline.encoder_fp16) with the layers named in wino_layers under the Winograd contract."""
    acts = {}
    x = q16(x)
    for name, s, p in opipe.ENCODER:
        w, b = params[name + "_weight"], params[name + "_bias"]
        if name in wino_layers:
            assert (s, p) == (1, 1) and w.shape[2:] == (3, 3), name
            x = np.asarray(conv_wino(x, w, b, opipe.SLOPE, q, acc), np.float32)
        else:
            x = q16(onet.conv2d(x, q16(w), b, s, p, opipe.SLOPE))
        acts[name] = x
    return acts


def refine_iteration(params, data, K, pixel_means_rev, T_means, T_stds, rot_coord, wino_layers):
    """oracle.pipeline.refine_iteration (pose branch) on the encoder above."""
    from oracle import se3, zoom
    x, zf = zoom.net_input(data["image_observed"], data["image_rendered"], data["mask_observed"], data["mask_rendered"],
                           data["src_pose"], K, pixel_means_rev, data.get("depth_observed"), data.get("depth_rendered"))
    out = {"net_input": x, "zoom_factor": zf}
    out.update(encoder(params, x, wino_layers))
    out["fc6"], out["fc7"], out["se3"] = opipe.pose_head(params, out["conv6_1"], zf)
    B = x.shape[0]
    pose = np.zeros((B, 3, 4))
    for b in range(B):
        pose[b] = se3.RT_transform(np.asarray(data["src_pose"][b], np.float32), out["se3"][b, :4], out["se3"][b, 4:], T_means,
                                   T_stds, rot_coord)
    out["pose_est"] = pose
    return out

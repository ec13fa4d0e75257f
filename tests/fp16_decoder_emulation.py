"""Emulation of the fp16 FlowNetS decoder and flow / mask heads (network.FP16_CONV with the decoder in the graph), composed from
oracle primitives. TEST INFRASTRUCTURE ONLY.

Arithmetic contract (`q` = round to fp16 and back):
  deconv5 / deconv4      q(lrelu(deconv(x, q(w)) + b))        into Concat2 / Concat3 channels [512, 512 + Cout)
  upsample_flow6to5/5to4 q(deconv(flow, w) + b)                fp32 flow in, one rounding at the store
  Convolution1/2/3,      conv(x, q(w)) + b                     fp32 NCHW out (products of two fp16 values are exact in fp32)
  mask_conv3
  Concat2 / Concat3 skip channels are the encoder's fp16 conv5_1 / conv4_1 as they are. With `q` the identity every function here is
  oracle.pipeline.decoder / mask_head / flow_head exactly (tests/test_fp16_decoder_emulation.py).
"""
import numpy as np

from oracle import net as onet
from oracle import pipeline as opipe

SLOPE = 0.1
q16 = opipe.q16


def nhwc_to_nchw(a):
    """(B,H,W,C) device read-back (any float dtype) → (B,C,H,W) float32."""
    return np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 3, 1, 2))


def deconv(params, name, x, Ho, Wo, slope, q=q16):
    """deconv5 / deconv4 as the fp16 path computes them: fp16 weights, one rounding of the activated result."""
    return q(onet.deconv4x4s2_crop(x, q(params[name + "_weight"]), params[name + "_bias"], Ho, Wo, (1, 1), slope))


def upsample_flow(params, name, flow, Ho, Wo, q=q16):
    return q(onet.deconv4x4s2_crop(flow, params[name + "_weight"], params[name + "_bias"], Ho, Wo, (1, 1), 1.0))


def predictor(params, name, x, q=q16):
    """Convolution1 / 2 / 3, mask_conv3: 3x3 pad 1, fp16 weights, fp32 result."""
    return onet.conv2d(x, q(params[name + "_weight"]), params[name + "_bias"], 1, 1, 1.0)


def decoder(params, acts, q=q16):
    """acts: conv4_1 / conv5_1 / conv6_1 (NCHW float32 holding the encoder's fp16 values) → flow6, Concat2, flow5, Concat3."""
    c6 = acts["conv6_1"]
    flow6 = predictor(params, "Convolution1", c6, q)
    d5 = deconv(params, "deconv5", c6, 15, 20, SLOPE, q)
    up6 = upsample_flow(params, "upsample_flow6to5", flow6, 15, 20, q)
    concat2 = np.concatenate([acts["conv5_1"], d5, up6], axis=1)
    flow5 = predictor(params, "Convolution2", concat2, q)
    d4 = deconv(params, "deconv4", concat2, 30, 40, SLOPE, q)
    up5 = upsample_flow(params, "upsample_flow5to4", flow5, 30, 40, q)
    concat3 = np.concatenate([acts["conv4_1"], d4, up5], axis=1)
    return {"flow6": flow6, "Concat2": concat2, "flow5": flow5, "Concat3": concat3}


def heads(params, concat3, zoom_factor, H, W, normalize_flow, mask=True, flow=True, q=q16):
    """mask / flow heads from Concat3: fp16-weight predictors, then the unchanged fp32 upsampling and inverse zoom."""
    qp = dict(params)
    for name in ("mask_conv3_weight", "Convolution3_weight"):
        if name in qp:
            qp[name] = q(qp[name])
    out = {}
    if mask:
        out["mask_lowres"], out["mask_logits"], out["mask_observed_pred"] = opipe.mask_head(qp, concat3, zoom_factor, H, W)
    if flow:
        out["flow_lowres"], out["zoom_flow_est"], out["flow_est"] = opipe.flow_head(qp, concat3, zoom_factor, H, W, normalize_flow)
    return out

"""FlowNetS-backboned matching network of DeepIM as a resident device pipeline.

Mirrors ``deepim/symbols/deepIM_flownet.py`` (reference): ``get_symbol`` / ``get_test_symbol_share``
(:548-735), ``get_convs`` (:32-169) and ``init_weights`` (:753-845) keep their names and the MXNet
parameter naming (``flow_conv1_weight`` ... ``trans_bias``), but instead of an MXNet Symbol the
"symbol" is a bound chain of HIP launches on one stream:

    zoom (ZoomMask + ZoomImageWithFactor [+ ZoomDepth] + /255 + Concat, one fused front end)
    → 10 × (Convolution + bias + LeakyReLU 0.1) on the fp32 matrix cores
    → fc6 → fc7 → rot/trans + inverse ZoomTrans → se3
    [→ FlowNetS refinement decoder → mask / flow heads when the config keeps them in the test graph]
    → RT_transform (pose update, lib/pair_matching/RT_transform.py:127-151)

All activations, weights and the per-iteration pre-staged frames stay in HBM; nothing crosses
PCIe inside the refinement loop.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

from ..config import ROT_COORD_CODE, X3_GRAD_SCALE_DEFAULT, X3_SCALE_WINDOW_DEFAULT, default_config
from ..runtime import Context, DeviceArray, lib

# name, Cout, kernel, stride, pad  (deepIM_flownet.py:63-107)
ENCODER = [
    ("flow_conv1", 64, 7, 2, 3),
    ("conv2", 128, 5, 2, 2),
    ("conv3", 256, 5, 2, 2),
    ("conv3_1", 256, 3, 1, 1),
    ("conv4", 512, 3, 2, 1),
    ("conv4_1", 512, 3, 1, 1),
    ("conv5", 512, 3, 2, 1),
    ("conv5_1", 512, 3, 1, 1),
    ("conv6", 1024, 3, 2, 1),
    ("conv6_1", 1024, 3, 1, 1),
]
SLOPE = 0.1


def _out_hw(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _pad8(c):       # the channels of an NHWC fp16 record: a multiple of 8
    return (c + 7) // 8 * 8


# The FlowNetS refinement decoder and the heads at the network's 480x640 input (deepIM_flownet.py:120-167, :183-207, :314-361), in
# the order of their parameters. kind: "pred" = 3x3 stride-1 predictor, "deconv" = 4x4 stride-2 Deconvolution + Crop(1,1) into
# channels [coff, coff + cout) of the Concat `out`, "bilinear" = the fixed 16x upsampling + Crop. head: the output that keeps the
# layer in the graph (None: either). slope 1.0: no activation.
_Layer = namedtuple("_Layer", "name kind head cin cout hw_in hw_out out coff slope")
DECODER = {l.name: l for l in (
    _Layer("Convolution1", "pred", None, 1024, 2, (8, 10), (8, 10), "flow6", 0, 1.0),
    _Layer("deconv5", "deconv", None, 1024, 512, (8, 10), (15, 20), "Concat2", 512, SLOPE),
    _Layer("upsample_flow6to5", "deconv", None, 2, 2, (8, 10), (15, 20), "Concat2", 1024, 1.0),
    _Layer("Convolution2", "pred", None, 1026, 2, (15, 20), (15, 20), "flow5", 0, 1.0),
    _Layer("deconv4", "deconv", None, 1026, 256, (15, 20), (30, 40), "Concat3", 512, SLOPE),
    _Layer("upsample_flow5to4", "deconv", None, 2, 2, (15, 20), (30, 40), "Concat3", 768, 1.0),
    _Layer("mask_conv3", "pred", "mask", 770, 1, (30, 40), (30, 40), "mask_lowres", 0, 1.0),
    _Layer("mask_upsampling", "bilinear", "mask", 1, 1, (30, 40), (480, 640), "mask_logits", 0, 1.0),
    _Layer("Convolution3", "pred", "flow", 770, 2, (30, 40), (30, 40), "flow_lowres", 0, 1.0),
    _Layer("upsampling", "bilinear", "flow", 2, 2, (30, 40), (480, 640), "zoom_flow_est", 0, 1.0),
)}
# Concat → (channels, (h, w), the encoder activation that is its first input, that one's channels): 1026 and 770 channels
SKIPS = {"Concat2": "conv5_1", "Concat3": "conv4_1"}
CONCAT = {cat: (max(l.coff + l.cout for l in DECODER.values() if l.out == cat),
                next(l.hw_out for l in DECODER.values() if l.out == cat), skip, {e[0]: e[1] for e in ENCODER}[skip])
          for cat, skip in SKIPS.items()}
FC6_IN = ENCODER[-1][1] * 8 * 10     # conv6_1 flattened

from .deepIM_flownet_train import TrainGraph  # noqa: E402  (the training mixin reads the tables above)


class _Activations(dict):
    """The activation buffers of a bound network. `act["net_input"]` is always the (B,C,H,W) tensor of the reference graph:
    when the zoom front end wrote the channel-blocked form for conv1 (8-channel input, NC8 encoder) it is converted into the
    NCHW buffer on demand — tests and the bench's parity taps read it, the hot path does not."""

    def __init__(self, net):
        dict.__init__(self)
        self._net = net

    def __getitem__(self, key):
        if key == "net_input" and self._net._input_live_h16:
            # fp16 mode: the front end wrote fp16 pixel records; their float values (exactly what conv1 multiplies) as NCHW
            n, h = self._net, self._net.ctx.handle
            out = dict.__getitem__(self, "net_input")
            if n.cin == 8:
                lib.deepim_nhwc_f16_to_nchw_f32(h, out, dict.__getitem__(self, "net_input_h8"), n.B, 8, n.H, n.W)
            else:
                if "net_input_tmp" not in self:
                    self["net_input_tmp"] = n.ctx.empty((n.B, 8, n.H, n.W))
                tmp = dict.__getitem__(self, "net_input_tmp")
                lib.deepim_nhwc_f16_to_nchw_f32(h, tmp, dict.__getitem__(self, "net_input_h8"), n.B, 8, n.H, n.W)
                lib.deepim_copy_channels(h, out, 10, 0, tmp, 8, n.B, n.H * n.W)
                lib.deepim_nhwc_f16_to_nchw_f32(h, tmp, dict.__getitem__(self, "net_input_x2"), n.B, 2, n.H, n.W)
                lib.deepim_copy_channels(h, out, 10, 8, tmp, 2, n.B, n.H * n.W)
        if key == "net_input" and self._net._input_live_nc8:
            out, src = dict.__getitem__(self, "net_input"), dict.__getitem__(self, "net_input_nc8")
            lib.deepim_relayout_nc8(self._net.ctx.handle, out, src, self._net.B, 8, self._net.H * self._net.W, 0)
        return dict.__getitem__(self, key)


class deepIM_flownet(TrainGraph):
    def __init__(self):
        self.cfg = None
        self.ctx = None
        self.B = 0
        self.params = {}    # name -> DeviceArray (raw MXNet-layout parameters)
        self.packed = {}    # conv/deconv name -> packed weights
        self.act = _Activations(self)
        # every flag and container the graph reads, with the value it has until get_symbol / bind / zoom / encoder say otherwise
        self.is_train = self.train_winograd = self.train_x3 = self.two_streams = False
        self.fp16_conv = self.x3_conv = self.fp16_decoder = self.fp16_winograd = self.fp16_fused_input = False
        self.conv1_nc8 = self.nc8 = self.winograd = False
        self.rot_type, self.rot_param, self.act_layout = "QUAT", 4, "nchw"    # (act_layout: as the last encoder() left the activations)
        self._input_live_h16 = self._input_live_nc8 = False        # set by zoom(): which form of the net input is the live one
        # the fp32 Winograd packs (_pack_wino, _pack_wino_dgrad)
        self.packed_wino, self.wino_s2d, self.wino_s2d3, self.wino_conv1, self.packed_wino_dgrad = {}, set(), {}, None, {}
        self._upd_ws = self._sgd_table = self._adam_table = None   # train_step's updater workspace, update()'s pointer tables

    # ------------------------------------------------------------------ graph description
    def get_symbol(self, cfg=None, is_train=False):
        if cfg is None:
            cfg = default_config()
        if cfg.network.REGRESSOR_NUM != 1:
            raise Exception("NOT IMPLEMENTED")  # deepIM_flownet.py:748
        self.cfg = cfg
        if is_train:
            return self.get_train_symbol(cfg)
        return self.get_test_symbol_share(cfg)

    def get_train_symbol(self, cfg):
        """Training graph (deepIM_flownet.py:367-546 with get_convs :32-169 and get_loss :170-365): zoom (region from
        mask_gt_observed) → encoder → fc6/fc7 → rot → L2Normalization, trans → inverse ZoomTrans → Transform3D →
        point-matching loss; with network.PRED_FLOW / PRED_MASK also the FlowNetS refinement decoder, Convolution3 →
        upsampling → flow loss against the ZoomFlow-ed labels, and mask_conv3 → mask_upsampling →
        LogisticRegressionOutput against the zoomed mask_gt_observed. forward_train / backward / update run all of it
        resident on the device."""
        n = cfg.network
        t = cfg.train_iter
        if not (t.SE3_PM_LOSS or t.get("SE3_DIST_LOSS", False)):
            raise NotImplementedError("training graph needs train_iter.SE3_PM_LOSS or train_iter.SE3_DIST_LOSS")
        if str(n.ROT_TYPE).upper() != "QUAT":
            # the reference's get_loss builds a 4-output rot head + L2Normalization whatever ROT_TYPE says (deepIM_flownet.py:211-217):
            # an EULER training graph does not exist there either — refuse instead of training the wrong head
            raise NotImplementedError("training graph: network.ROT_TYPE must be 'QUAT' (deepIM_flownet.py:211-217 is quaternion-only)")
        # rot / trans distance losses (deepIM_flownet.py:238-262)
        self.se3_dist_loss = bool(t.get("SE3_DIST_LOSS", False))
        self.se3_pm_loss = bool(t.SE3_PM_LOSS)
        self.trans_loss_type = str(t.get("TRANS_LOSS_TYPE", "L2"))
        if self.se3_dist_loss and self.trans_loss_type not in ("L2", "smooth_L1", "L1"):
            raise Exception("Does not support small_cfg.TRANS_LOSS_TYPE: {}".format(self.trans_loss_type))      # :258-259
        # TRAIN.optimizer (train.py:260-338): "sgd" = MXNet sgd_mom_update, "adam" = MXNet adam_update; update() dispatches on it
        # (the reference compares the strings exactly and trains nothing on any other value: refuse it)
        self.optimizer = cfg.TRAIN.get("optimizer", "sgd")
        if self.optimizer not in ("sgd", "adam"):
            raise ValueError("TRAIN.optimizer must be 'sgd' or 'adam', got {!r}".format(self.optimizer))
        if n.get("X3_CONV", False):
            # encoder_x3 fills only the split16 activations and no backward reads them
            raise NotImplementedError("training graph runs the fp32 or the fp16 convolutions only (network.X3_CONV unset)")
        # network.FP16_CONV: mixed precision, fp16 encoder forward and backward with a device-resident loss scale.
        # TRAIN.X3_CONV: split-fp16 encoder forward and backward with a device-resident gradient scale. The fp16
        # graph ignores the key, as it ignores TRAIN.WINOGRAD_CONV
        tr, fp16 = cfg.TRAIN, bool(n.get("FP16_CONV", False))
        train_x3 = bool(tr.get("X3_CONV", False)) and not fp16
        if train_x3 and tr.get("WINOGRAD_CONV", False):
            raise ValueError("TRAIN.X3_CONV and TRAIN.WINOGRAD_CONV exclude each other: one encoder arithmetic per training graph")
        if fp16 or train_x3:
            skey, sdef, wkey, wdef = ("FP16_LOSS_SCALE", 1024.0, "FP16_SCALE_WINDOW", 1000) if fp16 else \
                                     ("X3_GRAD_SCALE", X3_GRAD_SCALE_DEFAULT, "X3_SCALE_WINDOW", X3_SCALE_WINDOW_DEFAULT)
            self.loss_scale_init = self._check_loss_scale(tr.get(skey, sdef), "TRAIN." + skey)
            self.loss_scale_window = int(tr.get(wkey, wdef))
            if self.loss_scale_window < 1:
                raise ValueError("TRAIN.{} must be >= 1, got {}".format(wkey, self.loss_scale_window))
        self.get_test_symbol_share(cfg)
        self.train_x3 = train_x3
        if train_x3:
            self.x3_conv = True    # the forward of the x3 test graph: encoder_x3() on packed_x3 and the split16 activations
        self.fp16_decoder = False  # network.FP16_DECODER governs the test graph only: the training decoder and heads are fp32
        self.fp16_winograd = False  # network.FP16_WINOGRAD too: the backward differentiates the direct fp16 forward
        self.is_train = True
        # TRAIN.WINOGRAD_CONV: the forward of the inference encoder (channel-blocked activations, fp32 Winograd
        # layers) with a backward that reads those activations in place. The fp16 graph ignores the key
        self.train_winograd = bool(cfg.TRAIN.get("WINOGRAD_CONV", False)) and not self.fp16_conv
        self.nc8 = self.train_winograd   # False: NCHW activations, what the default backward kernels read
        self.two_streams = False  # backward(): weight gradients on a second stream next to the data gradients (False: one stream)
        self.with_mask_head, self.with_flow_head = bool(n.PRED_MASK), bool(n.PRED_FLOW)    # :183, :314
        self.with_decoder = self.with_mask_head or self.with_flow_head
        return self

    @staticmethod
    def _check_loss_scale(scale, key="TRAIN.FP16_LOSS_SCALE"):
        v = float(scale)
        if not (v >= 1.0 and v <= 2.0 ** 24 and np.isfinite(v) and np.frexp(v)[0] == 0.5):
            raise ValueError("{} must be a power of two in [1, 2^24], got {}".format(key, scale))
        return v

    def get_test_symbol_share(self, cfg):
        n = cfg.network
        self.input_mask = bool(n.INPUT_MASK)
        self.input_depth = bool(n.INPUT_DEPTH)
        self.update_mask = cfg.TEST.UPDATE_MASK
        # deepIM_flownet.py:624 / :676 — which heads stay in the test graph
        self.with_mask_head = bool(n.PRED_MASK) and (cfg.TEST.UPDATE_MASK not in ["init", "box_rendered"]
                                                     or not cfg.TEST.FAST_TEST)
        self.with_flow_head = bool(n.PRED_FLOW) and not cfg.TEST.FAST_TEST
        self.with_decoder = self.with_mask_head or self.with_flow_head
        self.cin = 6 + (2 if self.input_depth else 0) + (2 if self.input_mask else 0)
        # BASELINE config 5: conv stack on the fp16 matrix cores (NHWC fp16 activations, fp32 accumulate)
        self.fp16_conv = bool(n.get("FP16_CONV", False))
        # split-fp16 conv path: fp32-grade products (hi·hi + hi·lo + lo·hi, fp32 accumulation) on the fp16 matrix cores for
        # conv2 … conv6_1; conv1 stays on the fp32 kernel. Within the 1e-4 bar (observed ~1e-6), not bit-exact.
        self.x3_conv = bool(n.get("X3_CONV", False)) and not self.fp16_conv
        # fp16 conv path with the decoder in the graph: Concat2 / Concat3 stay NHWC fp16, deconv5 / deconv4 on the fp16 matrix cores,
        # the few-filter predictors from the fp16 concats (csrc/decoder_f16.hip). network.FP16_DECODER = False: the fp32 decoder
        # fed the encoder's fp16 activations converted to fp32 (the A/B baseline)
        self.fp16_decoder = self.fp16_conv and self.with_decoder and bool(n.get("FP16_DECODER", True))
        # fp16 conv path with the 3x3 stride-1 encoder layers as fp16 Winograd F(2x2,3x3) (csrc/wino_f16.hip): every layer the kernel
        # supports, no per-layer choice by speed. Its own arithmetic contract (about 1.5x the direct fp16 kernel's per-layer error)
        self.fp16_winograd = self.fp16_conv and bool(n.get("FP16_WINOGRAD", False))
        self.nc8 = bool(n.get("NC8_CONV", True))
        # the 3x3 stride-1 encoder layers as fp32 Winograd F(2x2,3x3) (csrc/wino.hip) wherever the layer fills the chip: same fp32
        # arithmetic, 2.25x fewer multiplies, a different summation (<= 1e-5 of the layer's range from the direct sum). Only on
        # the channel-blocked path; network.WINOGRAD_CONV = False keeps the direct kernels.
        self.winograd = bool(n.get("WINOGRAD_CONV", True))
        self.H, self.W = cfg.SCALES[0]
        self.K = np.ascontiguousarray(cfg.dataset.INTRINSIC_MATRIX, dtype=np.float32).reshape(3, 3)
        # Prop-side channel reversal of the means (zoom_image_with_factor.py:79-81)
        self.pixel_means = np.ascontiguousarray(np.asarray(n.PIXEL_MEANS, np.float32).reshape(3)[::-1])
        self.T_means = np.ascontiguousarray(cfg.dataset.trans_means, dtype=np.float32).reshape(3)
        self.T_stds = np.ascontiguousarray(cfg.dataset.trans_stds, dtype=np.float32).reshape(3)
        self.rot_coord = ROT_COORD_CODE[n.ROT_COORD.lower()]
        self.normalize_flow = float(cfg.dataset.NORMALIZE_FLOW)
        # deepIM_flownet.py:715: the rot head has 3 outputs for EULER, 4 otherwise; tester.py:391-398 hands rot_type to RT_transform
        self.rot_type = str(n.ROT_TYPE).upper()
        if self.rot_type not in ("QUAT", "EULER"):
            raise Exception("Unknown rot_type: {}".format(n.ROT_TYPE))          # RT_transform.py:142-143
        self.rot_param = 3 if self.rot_type == "EULER" else 4
        if self.rot_type == "EULER" and (self.fp16_conv or self.x3_conv):
            raise NotImplementedError("network.ROT_TYPE = 'EULER' runs on the fp32 convolution paths only")
        return self

    def arg_shape_dict(self):
        """MXNet parameter names → shapes (what `sym.infer_shape` reports for the weights)."""
        d = {}
        cin = self.cin
        for name, cout, k, s, p in ENCODER:
            d[name + "_weight"] = (cout, cin, k, k)
            d[name + "_bias"] = (cout,)
            cin = cout
        d["fc6_weight"], d["fc6_bias"] = (256, FC6_IN), (256,)
        d["fc7_weight"], d["fc7_bias"] = (256, 256), (256,)
        rp = self.rot_param                       # deepIM_flownet.py:715
        d["rot_weight"], d["rot_bias"] = (rp, 256), (rp,)
        d["trans_weight"], d["trans_bias"] = (3, 256), (3,)
        for l in self._decoder_layers():
            if l.kind == "bilinear":
                d[l.name + "_weight"] = (l.cout, 1, 32, 32)
            else:       # Convolution (cout, cin, 3, 3); Deconvolution, MXNet's (cin, cout, 4, 4)
                d[l.name + "_weight"] = (l.cout, l.cin, 3, 3) if l.kind == "pred" else (l.cin, l.cout, 4, 4)
                d[l.name + "_bias"] = (l.cout,)
        return d

    def _decoder_layers(self):
        """The rows of DECODER that this graph keeps."""
        keep = {None: self.with_decoder, "mask": self.with_mask_head, "flow": self.with_flow_head}
        return [l for l in DECODER.values() if keep[l.head]]

    @staticmethod
    def _init_bilinear(shape):
        """MXNet Initializer._init_bilinear (used at deepIM_flownet.py:808-822)."""
        w = np.zeros(int(np.prod(shape)), dtype=np.float32)
        f = np.ceil(shape[3] / 2.0)
        c = (2 * f - 1 - f % 2) / (2.0 * f)
        for i in range(w.size):
            x = i % shape[3]
            y = (i // shape[3]) % shape[2]
            w[i] = (1 - abs(x / f - c)) * (1 - abs(y / f - c))
        return w.reshape(shape)

    def init_weights(self, cfg=None, arg_params=None, aux_params=None, seed=2333, names=None):
        """Seeded synthetic parameters (no checkpoints offline): He-normal conv/FC so activations stay
        O(1) through the 10 layers, rot/trans as the reference initialises them
        (deepIM_flownet.py:795-803), bilinear upsampling kernels (:808-822)."""
        rng = np.random.default_rng(seed)
        arg_params = {} if arg_params is None else arg_params
        shapes = self.arg_shape_dict()
        self.adapt_checkpoint(arg_params, shapes)
        for name, shape in shapes.items():
            if name in arg_params or (names is not None and name not in names):   # `names`: only these (tests)
                continue
            if name.endswith("upsampling_weight"):
                arg_params[name] = self._init_bilinear(shape)
            elif name.endswith("_bias"):
                arg_params[name] = (0.01 * rng.standard_normal(shape)).astype(np.float32)
            elif name == "rot_weight" and self.rot_type == "EULER":
                arg_params[name] = np.zeros(shape, np.float32)      # deepIM_flownet.py:791-792
            elif name == "rot_weight":
                w = rng.random(shape) * 0.01
                w[0, :] = rng.random(shape[1]) + 0.01
                arg_params[name] = w.astype(np.float32)
            elif name == "trans_weight":
                arg_params[name] = (0.01 * rng.standard_normal(shape)).astype(np.float32)
            else:
                fan_in = int(np.prod(shape[1:]))
                if name.startswith("deconv") or name.startswith("upsample_flow"):
                    fan_in = shape[0] * 4  # 2x2 taps reach each output of a k4 s2 transposed conv
                gain = 2.0 / (1 + SLOPE ** 2)
                arg_params[name] = (rng.standard_normal(shape) * np.sqrt(gain / fan_in)).astype(np.float32)
        return arg_params

    @staticmethod
    def adapt_checkpoint(arg_params, shapes):
        """An RGB-pair (6-channel FlowNet) checkpoint under a graph with depth / mask inputs: the extra input channels of
        `flow_conv1_weight` start from zero weights (deepIM_flownet.py:759-773). In place; returns arg_params."""
        w1 = arg_params.get("flow_conv1_weight")
        if w1 is not None and w1.shape[1] < shapes["flow_conv1_weight"][1]:
            w1 = np.asarray(w1.asnumpy() if hasattr(w1, "asnumpy") else w1, dtype=np.float32)
            extra = shapes["flow_conv1_weight"][1] - w1.shape[1]
            arg_params["flow_conv1_weight"] = np.concatenate(
                [w1, np.zeros((w1.shape[0], extra) + w1.shape[2:], np.float32)], axis=1)
        return arg_params

    # ------------------------------------------------------------------ bind
    def bind(self, ctx: Context, batch_size: int, arg_params: dict):
        assert self.cfg is not None, "call get_symbol first"
        self.ctx, self.B = ctx, int(batch_size)
        B, H, W = self.B, self.H, self.W
        shapes = self.arg_shape_dict()
        for name, shape in shapes.items():
            assert name in arg_params, name
            a = np.ascontiguousarray(arg_params[name], dtype=np.float32)
            assert tuple(a.shape) == tuple(shape), (name, a.shape, shape)
            self.params[name] = ctx.array(a)
        hh, ww, cin = H, W, self.cin
        self.enc_geom = []
        for name, cout, k, s, p in ENCODER:
            self.enc_geom.append((name, cin, hh, ww, cout, k, s, p))
            (hh, ww), cin = _out_hw(hh, ww, k, s, p), cout
        # one-time weight re-layout into MFMA operand order: every _pack_* below sizes, allocates and fills its buffers here, and
        # refills them for update() after an optimizer step
        for base in self._direct_layers():
            self._pack_direct(base, True)
        self.packed_wino, self.wino_s2d, self.wino_s2d3, self.wino_conv1, self.packed_wino_dgrad = {}, set(), {}, None, {}
        if self.nc8 and self.winograd and not (self.fp16_conv or self.x3_conv) and (not self.is_train or self.train_winograd):
            self._pack_wino(True)
        self._pack_fc6(True)
        if self.fp16_conv:
            self.packed_f16 = {}
            self._pack_f16(True)
        if self.x3_conv:
            self.packed_x3, self.x3_wscale = {}, {}
            self._pack_x3(True, arg_params)
        # activations
        A, f16 = self.act, np.float16
        A["net_input"], A["zoom_factor"] = ctx.empty((B, self.cin, H, W)), ctx.empty((B, 4))
        for name, cin, hh, ww, cout, k, s, p in self.enc_geom:
            ho, wo = _out_hw(hh, ww, k, s, p)
            A[name] = ctx.empty((B, cout, ho, wo))
            if self.fp16_conv:
                A[name + "_h"] = ctx.empty((B, ho, wo, cout), dtype=f16)   # NHWC fp16
            if self.x3_conv:
                A[name + "_x"] = ctx.empty((B, ho, wo, 2 * cout), dtype=f16)   # split16 NHWC
        if self.fp16_conv:
            self.cin_pad = _pad8(self.cin)
            A["net_input_h"] = ctx.empty((B, H, W, self.cin_pad), dtype=f16)
            if "conv1_patch" in self.packed_f16 and self.input_mask:
                # the zoom front end writes conv1's fp16 pixel records itself (no fp32 net input, no conversion pass);
                # `net.fp16_fused_input = False` restores the two-step form for A/B measurements
                A["net_input_h8"] = ctx.empty((B, H, W, 8), dtype=f16)
                if self.cin == 10:
                    A["net_input_x2"] = ctx.empty((B, H, W, 2), dtype=f16)
                self.fp16_fused_input = True
        self._input_live_h16 = self._input_live_nc8 = False
        A["fc6"], A["fc7"], A["se3"] = ctx.empty((B, 256)), ctx.empty((B, 256)), ctx.empty((B, self.rot_param + 3))
        if self.rot_type == "EULER":
            A["rot_e"], A["zoom_trans_e"], A["trans_e"] = ctx.empty((B, 3)), ctx.empty((B, 3)), ctx.empty((B, 3))
        A["pose_est"] = ctx.empty((B, 3, 4))
        self.heads16 = [l.name for l in self._decoder_layers() if l.kind == "pred" and l.head]   # the predictors on Concat3
        for l in self._decoder_layers():       # flow6 / flow5 / mask_lowres / flow_lowres, mask_logits / zoom_flow_est
            if l.kind != "deconv":
                A[l.out] = ctx.empty((B, l.cout) + l.hw_out)
        for cat, (ctotal, hw, _skip, _cs) in CONCAT.items() if self.with_decoder else ():
            if self.fp16_decoder:
                # NHWC fp16 concats, channels padded to a multiple of 8; the pad channels are zeroed here, once, and never written
                A[cat + "_h"] = ctx.zeros((B,) + hw + (_pad8(ctotal),), dtype=f16)
            else:
                A[cat] = ctx.empty((B, ctotal) + hw)
        if self.fp16_decoder:
            self._pack_dec16()
        if self.with_mask_head:
            A["mask_observed_pred"] = ctx.empty((B, 1, H, W))
        if self.with_flow_head:
            A["flow_est"] = ctx.empty((B, 2, H, W))
        ctx.sync()
        return self

    # Concat2 (1026 channels) / Concat3 (770) as NHWC fp16 records: multiples of 8
    CONCAT2_H, CONCAT3_H = _pad8(CONCAT["Concat2"][0]), _pad8(CONCAT["Concat3"][0])

    # ------------------------------------------------------------------ weight packs: one function per buffer family
    def _pack(self, store, key, alloc, size_args, pack, *pack_args, dtype=np.float32):
        """Fill the packed buffer store[key] through the library's entry `pack` (deepim_<kernel>_pack_weights[_<variant>]); with
        `alloc` (bind) first make it, of the bytes that kernel's deepim_<kernel>_packed_size(*size_args) names. bind() and update()
        both come through here, so a buffer has one size and one pack call."""
        if alloc:
            nb = getattr(lib.load(), pack.split("_pack_weights")[0] + "_packed_size")(*size_args)
            store[key] = DeviceArray(self.ctx, (nb // np.dtype(dtype).itemsize,), dtype)
        getattr(lib, pack)(self.ctx.handle, store[key], *pack_args)

    def _direct_layers(self):
        """The conv / deconv layers with an entry in `packed`, in parameter order: all but the fixed bilinear kernels."""
        return [g[0] for g in self.enc_geom] + [l.name for l in self._decoder_layers() if l.kind != "bilinear"]

    def _pack_direct(self, base, alloc, order=None):
        """packed[base] in MFMA tile order. A convolution gets every operand order at bind and, after an optimizer step, only
        `order`: the one its forward reads in the training graph (_train_pack_orders)."""
        w = self.params[base + "_weight"]
        if base.startswith("deconv") or base.startswith("upsample_flow"):
            self._pack(self.packed, base, alloc, w.shape[:2], "deepim_deconv_pack_weights", w, *w.shape[:2])
        elif order is None:
            self._pack(self.packed, base, alloc, w.shape, "deepim_conv_pack_weights", w, *w.shape)
        else:
            self._pack(self.packed, base, alloc, w.shape, "deepim_conv_pack_weights_ex", w, *w.shape, order)

    def _pack_fc6(self, alloc):
        """packed["fc6"]: the 84 MB weight in MFMA operand order, so the layer is one pass over the weights on the matrix cores."""
        self._pack(self.packed, "fc6", alloc, (256, FC6_IN), "deepim_fc_pack_weights", self.params["fc6_weight"], 256, FC6_IN)

    def _wino_kind(self, li, alloc):
        """The fp32 Winograd pack of encoder layer li. "wino": 3x3 stride 1 as F(2x2,3x3). "s2d": 5x5 stride 2 = stride 1 over the
        four input phases (the layer before writes its output space-to-depth). "s2d3": conv4 / conv5 / conv6, the 3x3 kernel as
        taps 1..3 of a 5x5 stride-2 one over the same space-to-depth input (25 of the 64 (phase, position) GEMMs live). "conv1":
        7x7 stride 2 as F(2x2,4x4) over its four input phases (csrc/wino_c1.hip). None: the direct kernel. At bind the library's
        `preferred` answers choose; after an optimizer step it is the kernel that
        encoder_layer() picks now, asked the way it asks: the context's options may have changed since bind."""
        name, cin, hh, ww, cout, k, s_, p_ = self.enc_geom[li]
        L, q = lib.load(), (self.ctx.handle, self.B, cin, hh, ww, cout)
        if not alloc:
            if self._s2d3_live(li):
                return "s2d3"
            if name in self.packed_wino:
                return "s2d" if name in self.wino_s2d else "wino"
            return "conv1" if li == 0 and self.wino_conv1 is not None and L.deepim_conv1_wino_preferred(*q) else None
        kind, preferred = {(7, 2, 3): ("conv1", L.deepim_conv1_wino_preferred), (3, 1, 1): ("wino", L.deepim_conv_wino_preferred),
                           (5, 2, 2): ("s2d", L.deepim_conv_wino_preferred_s2d), (3, 2, 1): ("s2d3", L.deepim_conv_wino_preferred_s2d3)}[k, s_, p_]
        return kind if preferred(*q) else None

    def _pack_wino(self, alloc):
        """The channel-blocked fp32 encoder's weights. Bind: the Winograd packs, next to `packed`. After an optimizer step
        (TRAIN.WINOGRAD_CONV): per layer the one form the forward reads now — its Winograd pack, else the direct kernel's operand
        order for channel-blocked input (conv1 on the NCHW net input: the NCHW orders). packed_wino [+ wino_s2d] mean F(2x2,3x3)
        layers of 16 / 49 positions to bench.py's accounting, so the s2d3 layers and conv1 have attributes of their own."""
        n = len(self.enc_geom)
        for li in ([*range(1, n), 0] if alloc else range(n)):       # (bind asks about conv1 last)
            name, cin, _h, _w, cout = self.enc_geom[li][:5]
            kind, w = self._wino_kind(li, alloc), self.params[name + "_weight"]
            if kind == "conv1":
                self._pack(vars(self), "wino_conv1", alloc, (), "deepim_conv1_wino_pack_weights", w)
            elif kind is not None:
                self._pack(self.wino_s2d3 if kind == "s2d3" else self.packed_wino, name, alloc, (cout, cin if kind == "wino" else 4 * cin),
                           "deepim_conv_wino_pack_weights" + ("" if kind == "wino" else "_" + kind), w, cout, cin)
                if kind == "s2d":
                    self.wino_s2d.add(name)
            elif not alloc:
                self._pack_direct(name, False, 4 if li > 0 else 3)

    def _pack_wino_dgrad(self, alloc):
        """packed_wino_dgrad (TRAIN.WINOGRAD_CONV): U' of the 3x3 stride-1 data gradients on the Winograd kernels."""
        L, h, B = lib.load(), self.ctx.handle, self.B
        for name, cin, hh, ww, cout, k, s_, p_ in self.enc_geom[1:]:
            if name in self.packed_wino_dgrad or (alloc and (k, s_, p_) == (3, 1, 1) and cin % 32 == 0
                                                  and L.deepim_conv_wino_preferred(h, B, cout, hh, ww, cin)):
                self._pack(self.packed_wino_dgrad, name, alloc, (cin, cout), "deepim_conv_wino_pack_weights_dgrad",
                           self.params[name + "_weight"], cout, cin)

    def _pack_f16(self, alloc):
        """packed_f16: the fp16 weights in MFMA octet order from the fp32 masters, and conv1's pack for the patch kernel
        ("conv1_patch") where that one runs: the 8-channel input, or RGB-D (config 5) as the 8 + 2 channel form of the same kernel."""
        P, f16 = self.params, np.float16
        for name, cin, _h, _w, cout, k, _s, _p in self.enc_geom:
            self._pack(self.packed_f16, name, alloc, (cout, _pad8(cin), k, k), "deepim_conv_f16_pack_weights", P[name + "_weight"],
                       cout, cin, _pad8(cin), k, k, dtype=f16)
        w1 = P[ENCODER[0][0] + "_weight"]
        if self.cin in (8, 10) and self.W % 4 == 0:
            pack = ("deepim_conv1_x3_pack_weights", w1, ctypes.c_float(1.0)) if self.cin == 8 else ("deepim_conv1_f16_c10_pack_weights", w1)
            self._pack(self.packed_f16, "conv1_patch", alloc, (), *pack, dtype=f16)
        if not (alloc and self.fp16_winograd):
            return
        # packed_f16_wino (network.FP16_WINOGRAD, test graph only): transformed fp16 weights U = f16(G f16(w) G^T) in MFMA operand
        # order for every 3x3 stride-1 layer the kernel supports
        self.packed_f16_wino, self.fp16_wino_layers = {}, []
        for name, cin, _h, _w, cout, k, s_, p_ in self.enc_geom:
            if (k, s_, p_) == (3, 1, 1) and lib.load().deepim_conv_wino_f16_supported(cin, cout):
                self._pack(self.packed_f16_wino, name, True, (cout, cin), "deepim_conv_wino_f16_pack_weights",
                           self.params[name + "_weight"], cout, cin, dtype=np.float16)
                self.fp16_wino_layers.append(name)

    def _pack_x3(self, alloc, host_params=None):
        """packed_x3: split-fp16 weights [hi 16 | lo 16] in MFMA octet order, scaled by a power of two (x3_wscale) into fp16's range.
        conv1 only on the split-fp16 patch kernel (8-channel input; otherwise it stays fp32). The scales come from the host
        parameters at bind and stay: recomputing them would sync the host. A weight that has outgrown its scale is clamped by the
        pack; after an optimizer step the range check raises the overflow word for it, so the next step is skipped and reported."""
        for li, (name, cin, _h, _w, cout, k, _s, _p) in enumerate(self.enc_geom):
            if li == 0 and not (self.cin == 8 and self.W % 4 == 0):
                continue
            if alloc:
                m = float(np.abs(np.asarray(host_params[name + "_weight"], np.float32)).max())
                self.x3_wscale[name] = 2.0 ** int(np.floor(np.log2(1536.0 / m))) if m > 0 else 1.0
            w, sw = self.params[name + "_weight"], ctypes.c_float(self.x3_wscale[name])
            geo = () if li == 0 else (cout, cin, k, k)       # (the patch kernel's pack is conv1's own: no geometry)
            self._pack(self.packed_x3, name, alloc, geo, "deepim_conv1_x3_pack_weights" if li == 0 else "deepim_conv_x3_pack_weights", w,
                       *geo, sw, dtype=np.float16)
            if not alloc:
                lib.deepim_x3_weight_range_check(self.ctx.handle, w, w.size, sw, self.amp_state)

    def _pack_dec16(self):
        """packed_dec16 (fp16 decoder, test graph only): the fp16 packs of deconv5 / deconv4 and of the few-filter predictors. The
        heads share one pass over Concat3 (heads16): mask_conv3 first, then Convolution3, whichever of them the graph keeps."""
        P, f16 = self.params, np.float16
        self.packed_dec16 = {}
        for l in (DECODER["deconv5"], DECODER["deconv4"]):
            self._pack(self.packed_dec16, l.name, True, (_pad8(l.cin), l.cout), "deepim_deconv_f16_pack_weights",
                       P[l.name + "_weight"], l.cin, _pad8(l.cin), l.cout, dtype=f16)
        for key, names in (("Convolution1", ["Convolution1"]), ("Convolution2", ["Convolution2"]), ("heads", self.heads16)):
            l0, l1 = DECODER[names[0]], (DECODER[names[1]] if len(names) > 1 else None)
            self._pack(self.packed_dec16, key, True, (_pad8(l0.cin),), "deepim_fewout_f16_pack_weights", P[l0.name + "_weight"], l0.cout,
                       P[l1.name + "_weight"] if l1 else None, l1.cout if l1 else 0, l0.cin, _pad8(l0.cin), dtype=f16)

    def _fewout16(self, key, names, src):
        """One or two 3x3 predictors (DECODER rows `names`) in one pass over the NHWC fp16 tensor `src`."""
        A, P = self.act, self.params
        l0, l1 = DECODER[names[0]], (DECODER[names[1]] if len(names) > 1 else None)
        ctotal = _pad8(l0.cin)
        lib.deepim_conv3x3_fewout_f16_forward(self.ctx.handle, A[l0.out], l0.cout, A[l1.out] if l1 else None, l1.cout if l1 else 0, src,
                                              self.packed_dec16[key], P[l0.name + "_bias"], P[l1.name + "_bias"] if l1 else None,
                                              self.B, l0.hw_in[0], l0.hw_in[1], ctotal, ctotal)

    def _concat16(self, cat, src, flow):
        """One NHWC fp16 concat (padded to a multiple of 8 channels): [skip activation | lrelu(deconv(src)) | upsampled flow | 0]."""
        A, h, B, P = self.act, self.ctx.handle, self.B, self.params
        ctotal, (ho, wo), skip, cskip = CONCAT[cat]
        dec, up = [l for l in DECODER.values() if l.out == cat]
        cpad, out = _pad8(ctotal), A[cat + "_h"]
        lib.deepim_copy_channels_nhwc_f16(h, out, cpad, 0, A[skip + "_h"], cskip, 0, cskip, B * ho * wo)
        lib.deepim_deconv4x4s2_crop_f16_forward(h, out, src, self.packed_dec16[dec.name], P[dec.name + "_bias"], B, _pad8(dec.cin),
                                                _pad8(dec.cin), dec.hw_in[0], dec.hw_in[1], dec.cout, ho, wo, ctypes.c_float(dec.slope),
                                                cpad, dec.coff)
        lib.deepim_upsample_flow_f16_forward(h, out, A[flow], P[up.name + "_weight"], P[up.name + "_bias"], B, up.hw_in[0],
                                             up.hw_in[1], ho, wo, cpad, up.coff)

    # ------------------------------------------------------------------ forward pieces
    def _conv(self, name, src, dst, B, cin, h, w, cout, k, s, p, slope, ctotal=0, coff=0):
        lib.deepim_conv2d_forward(self.ctx.handle, dst, src, self.packed[name], self.params[name + "_bias"], B, cin, h,
                                  w, cout, k, k, s, p, ctypes.c_float(slope), ctotal, coff)

    def _pred(self, name, src):
        """The 3x3 predictor `name` of DECODER from `src` into its own activation."""
        l = DECODER[name]
        self._conv(name, src, self.act[l.out], self.B, l.cin, l.hw_in[0], l.hw_in[1], l.cout, 3, 1, 1, l.slope)

    def _deconv(self, name, src):
        """The transposed convolution `name` of DECODER from `src` into its channels of its Concat."""
        l = DECODER[name]
        lib.deepim_deconv4x4s2_crop_forward(self.ctx.handle, self.act[l.out], src, self.packed[name], self.params[name + "_bias"],
                                            self.B, l.cin, l.hw_in[0], l.hw_in[1], l.cout, l.hw_out[0], l.hw_out[1], 1, 1,
                                            ctypes.c_float(l.slope), CONCAT[l.out][0], l.coff)

    def _conv1_from_nc8(self):
        """OPT-IN (`net.conv1_nc8 = True` after bind; default off): conv1 reads a channel-blocked net input written by the
        zoom front end — the shipped 8-channel graph on the NC8 fp32 encoder (not the fp16 / x3 modes, which convert the NCHW
        input themselves, and not the training graph, whose backward reads NCHW). Measured in round 3 (profiles/r03_conv1_nc8.md):
        conv1 1.016 ms vs 1.006 ms on the NCHW register-fed kernel and the front end 0.179 vs 0.149 ms — conv1 is bound by its
        short K loop (49 tap groups per tile), not by the gather shape, so the default stays NCHW."""
        return (self.conv1_nc8 and self.nc8 and self.cin == 8 and self.input_mask and not self.input_depth
                and not self.fp16_conv and not self.x3_conv and not self.is_train and self.W % 4 == 0)

    def _render_boxes(self, data):
        """The boxes of this batch's two masks as update_test_batch left them (data["zoom_boxes"]), or None: search the masks.
        They are used only for the very mask objects that render call wrote (identity, not address: a caller that swaps a mask
        gets it searched), with TEST.UPDATE_MASK == "box_rendered" and network.INPUT_MASK. The first iteration, pre-staged
        frames and UPDATE_MASK == "init" carry no boxes."""
        boxes = data.get("zoom_boxes")
        wrote = getattr(boxes, "masks", None)
        if (boxes is None or wrote is None or not self.input_mask or getattr(self, "update_mask", None) != "box_rendered"
                or boxes.shape != (self.B, 2, 4) or boxes.dtype != np.int32):
            return None
        if data.get("mask_observed") is not wrote[0] or data.get("mask_rendered") is not wrote[1]:
            return None
        return boxes

    def zoom(self, data):
        """The fused zoom front end: this iteration's network input and zoom factor. Two independent choices.
        (With the masks of update_test_batch still in place, the two mask boxes come from that render pass: _render_boxes.)
        Observed source: the per-pair fp32 tensors, or a shared-frame batch (data["observed_frames"], lib/utils/image.ObservedFrames)
        whose observed image [and depth] are gathered from the N uint8 / uint16 frames through the device frame_index; the library
        refuses the mask-less ZoomImage configuration there.
        Output form: conv1's fp16 pixel records on the fused fp16 path, the opt-in NC8 records (_conv1_from_nc8; per-pair tensors
        only, there is no shared-frame variant), else the NCHW net input that the fp32, x3 and two-step fp16 encoders read.
        Camera: the run's `self.K`, or — with data["intrinsics"], a DeviceArray (B,3,3) — pair b's own row: the table is bound
        (Context.bind_cameras) and the entry gets NULL, in every form."""
        A, h, raw = self.act, self.ctx.handle, dict.__getitem__
        K = self.K
        cams = data.get("intrinsics")
        if cams is not None:
            if not isinstance(cams, DeviceArray) or cams.shape != (self.B, 3, 3):
                raise ValueError("data['intrinsics'] must be a DeviceArray (%d,3,3)" % self.B)
            self.ctx.bind_cameras(cams)
            K = None
        of = data.get("observed_frames")
        if of is not None and of.n_pairs != self.B:
            raise ValueError("observed_frames index %d pairs; the network is bound for %d" % (of.n_pairs, self.B))
        if of is not None and self.input_depth and of.depth is None:
            raise ValueError("network.INPUT_DEPTH: the observed_frames of this batch carry no depth frames")
        if self.fp16_conv and self.fp16_fused_input and "net_input_h8" in A:
            form, out = "h16", (raw(A, "net_input_h8"), raw(A, "net_input_x2") if self.cin == 10 else None)
        elif of is None and self._conv1_from_nc8():
            if "net_input_nc8" not in A:       # opt-in path: allocated on first use (run once eagerly before a graph capture)
                A["net_input_nc8"] = self.ctx.empty((self.B, self.H, self.W, 8))
            form, out = "nc8", (raw(A, "net_input_nc8"),)
        else:
            form, out = "nchw", (raw(A, "net_input"),)
        self._input_live_h16, self._input_live_nc8 = form == "h16", form == "nc8"
        masks = (data["mask_observed"], data["mask_rendered"]) if self.input_mask else (None, None)
        depth_rendered = data.get("depth_rendered") if self.input_depth else None
        if of is not None:
            depth = of.depth if self.input_depth else None
            labels, idx = (of.labels, of.mask_idx) if depth is not None else (None, None)
            entry = lib.deepim_zoom_concat_frames_forward_h16 if form == "h16" else lib.deepim_zoom_concat_frames_forward
            src = (of.image, of.frame_index, of.n_frames, data["image_rendered"]) + masks + \
                  (depth, labels, idx, ctypes.c_float(of.depth_factor), depth_rendered)
        else:
            entry = {"h16": lib.deepim_zoom_concat_forward_h16, "nc8": lib.deepim_zoom_concat_forward_nc8,
                     "nchw": lib.deepim_zoom_concat_forward}[form]
            depths = () if form == "nc8" else (data.get("depth_observed") if self.input_depth else None, depth_rendered)
            src = (data["image_observed"], data["image_rendered"]) + masks + depths
        boxes = self._render_boxes(data)
        if boxes is not None:      # one-shot: taken by the entry below, which then runs no bbox pass (cleared even if it fails)
            lib.deepim_zoom_seed_boxes(h, boxes)
        entry(h, *(src + (data["src_pose"], K, self.pixel_means) + out + (A["zoom_factor"], self.B, self.H, self.W)))

    def encoder_fp16(self):
        """Same 10 layers on the fp16 matrix cores: NCHW fp32 net input → NHWC fp16 → convs → conv6_1 back to
        NCHW fp32 for the (fp32) FC head."""
        A, h, B = self.act, self.ctx.handle, self.B
        geom = self.enc_geom
        if "conv1_patch" in self.packed_f16:
            name = geom[0][0]
            if self._input_live_h16:
                lib.deepim_conv1_f16_h16_forward(h, A[name + "_h"], dict.__getitem__(A, "net_input_h8"),
                                                 dict.__getitem__(A, "net_input_x2") if self.cin == 10 else None,
                                                 self.packed_f16["conv1_patch"], self.params[name + "_bias"], B, self.H, self.W,
                                                 ctypes.c_float(SLOPE))
            else:
                conv1 = lib.deepim_conv1_f16_c10_forward if self.cin == 10 else lib.deepim_conv1_f16_forward
                conv1(h, A[name + "_h"], A["net_input"], self.packed_f16["conv1_patch"], self.params[name + "_bias"], B, self.H,
                      self.W, ctypes.c_float(SLOPE))
            src, geom = A[name + "_h"], geom[1:]
        else:
            lib.deepim_nchw_f32_to_nhwc_f16(h, A["net_input_h"], A["net_input"], B, self.cin, self.H, self.W, self.cin_pad)
            src = A["net_input_h"]
        wino = self.packed_f16_wino if self.fp16_winograd else {}
        for name, cin, hh, ww, cout, k, s, p in geom:
            if name in wino:     # network.FP16_WINOGRAD: same tensors, the Winograd contract of csrc/wino_f16.hip
                lib.deepim_conv2d_wino_f16_forward(h, A[name + "_h"], src, wino[name], self.params[name + "_bias"], B, cin, hh, ww,
                                                   cout, ctypes.c_float(SLOPE))
            else:
                lib.deepim_conv2d_f16_forward(h, A[name + "_h"], src, self.packed_f16[name], self.params[name + "_bias"], B,
                                              _pad8(cin), hh, ww, cout, k, k, s, p, ctypes.c_float(SLOPE))
            src = A[name + "_h"]
        lib.deepim_nhwc_f16_to_nchw_f32(h, A["conv6_1"], src, B, 1024, 8, 10)

    X3_ACT_SCALE = 16.0   # stored split16 activations = value · 16: full 22-bit pairs down to |v| = 2^-6, saturation at 3750

    def encoder_x3(self):
        """The 10 layers with conv2 … conv6_1 on the split-fp16 kernel: conv1 in fp32 (NCHW) → split16 NHWC → 9 x3 convs →
        conv6_1 back to NCHW fp32 for the FC head."""
        A, h, B = self.act, self.ctx.handle, self.B
        c, sa = ctypes.c_float, self.X3_ACT_SCALE
        name, cin, hh, ww, cout, k, s, p = self.enc_geom[0]
        if name in self.packed_x3:
            lib.deepim_conv1_x3_forward(h, A[name + "_x"], A["net_input"], self.packed_x3[name], self.params[name + "_bias"], B,
                                        hh, ww, c(SLOPE), c(sa), c(1.0 / (sa * self.x3_wscale[name])), c(sa))
        else:
            lib.deepim_conv2d_forward_split16(h, A[name + "_x"], A["net_input"], self.packed[name], self.params[name + "_bias"],
                                              B, cin, hh, ww, cout, k, k, s, p, c(SLOPE), c(sa))
        src = A[name + "_x"]
        for name, cin, hh, ww, cout, k, s, p in self.enc_geom[1:]:
            lib.deepim_conv2d_x3_forward(h, A[name + "_x"], src, self.packed_x3[name], self.params[name + "_bias"], B, cin, hh,
                                         ww, cout, k, k, s, p, c(SLOPE), c(1.0 / (sa * self.x3_wscale[name])), c(sa))
            src = A[name + "_x"]
        lib.deepim_split16_to_nchw_f32(h, A["conv6_1"], src, B, 1024, 8, 10, c(1.0 / sa))
        self.act_layout = "x3"

    def encoder(self):
        """10 conv layers. With `self.nc8` (default) the layers hand each other channel-blocked activations
        ([n][C/8][h][w][8]): conv1 reads the NCHW net input and writes NC8, conv6_1 returns to NCHW for fc6 (MXNet's
        flatten order); `self.act[name]` of the layers in between then holds NC8 data (`activation_nchw` converts).
        `self.nc8 = False` keeps NCHW throughout (the canonical-order, bit-exact configuration of the tests)."""
        if self.fp16_conv:
            return self.encoder_fp16()
        if self.x3_conv:
            return self.encoder_x3()
        A = self.act
        src = self.conv1_input()
        for li in range(len(self.enc_geom)):
            self.encoder_layer(li, src)
            src = A[self.enc_geom[li][0]]
        self.act_layout = "nc8" if self.nc8 else "nchw"

    def conv1_input(self):
        """What conv1 reads: the channel-blocked (B,H,W,8) records when the last zoom() wrote them, else the NCHW net input."""
        if self._input_live_nc8:
            return dict.__getitem__(self.act, "net_input_nc8")
        return dict.__getitem__(self.act, "net_input")

    def encoder_layer(self, li, src):
        """One encoder conv (index into enc_geom) from `src` into its activation buffer, in the configured layout."""
        name, cin, h, w, cout, k, s, p = self.enc_geom[li]
        out_mode = self._enc_out_mode(li)
        if self._s2d3_live(li):
            # the 256-channel x 32-tile blocks where they measured faster (asked per call, as `_s2d3_live`: the options may change after bind)
            wide = lib.load().deepim_conv_wino_preferred_s2d3_wide(self.ctx.handle, self.B, cin, h, w, cout)
            fwd = lib.deepim_conv2d_wino_forward_s2d3_wide if wide else lib.deepim_conv2d_wino_forward_s2d3
            fwd(self.ctx.handle, self.act[name], src, self.wino_s2d3[name], self.params[name + "_bias"],
                self.B, cin, h, w, cout, ctypes.c_float(SLOPE), out_mode, 0, 0)
        elif self.nc8 and name in self.packed_wino:
            fwd = lib.deepim_conv2d_wino_forward_s2d if name in self.wino_s2d else lib.deepim_conv2d_wino_forward
            fwd(self.ctx.handle, self.act[name], src, self.packed_wino[name], self.params[name + "_bias"],      # s2d: 5x5 stride 2 over
                self.B, cin, h, w, cout, ctypes.c_float(SLOPE), out_mode, 0, 0)                                  # the space-to-depth tensor
        elif (self.nc8 and li == 0 and self.wino_conv1 is not None and src.shape != (self.B, self.H, self.W, 8)
              and lib.load().deepim_conv1_wino_preferred(self.ctx.handle, self.B, cin, h, w, cout)):
            # (asked again per call: a context switched to the canonical order after bind keeps conv1 on the direct kernel)
            lib.deepim_conv1_wino_forward(self.ctx.handle, self.act[name], src, self.wino_conv1, self.params[name + "_bias"],
                                          self.B, h, w, ctypes.c_float(SLOPE), out_mode)
        elif self.nc8:
            in8 = 1 if (li > 0 or src.shape == (self.B, self.H, self.W, 8)) else 0     # conv1: NC8 records from the zoom front end
            lib.deepim_conv2d_forward_ex(self.ctx.handle, self.act[name], src, self.packed[name], self.params[name + "_bias"],
                                         self.B, cin, h, w, cout, k, k, s, p, ctypes.c_float(SLOPE), 0, 0,
                                         in8, out_mode)
        else:
            self._conv(name, src, self.act[name], self.B, cin, h, w, cout, k, s, p, SLOPE)

    def _s2d3_live(self, li):
        """Whether encoder layer li (a 3x3 stride-2 layer bound in `wino_s2d3`) runs on the space-to-depth Winograd path now:
        `preferred` is asked again per call, so a context switched to the canonical order after bind keeps it on the direct kernel."""
        name, cin, h, w, cout = self.enc_geom[li][:5]
        return (self.nc8 and name in self.wino_s2d3
                and bool(lib.load().deepim_conv_wino_preferred_s2d3(self.ctx.handle, self.B, cin, h, w, cout)))

    def _enc_out_mode(self, li):
        """Output layout of encoder layer li on the channel-blocked path: 0 = NCHW (the last layer, for fc6), 3 = NC8 in
        space-to-depth order (the next layer is a stride-2 Winograd layer), 1 = NC8."""
        if li == len(self.enc_geom) - 1:
            return 0
        nxt = self.enc_geom[li + 1][0]
        if self.nc8 and nxt in self.wino_s2d and nxt in self.packed_wino:
            return 3
        return 3 if self._s2d3_live(li + 1) else 1

    def activation_nchw(self, name):
        """Encoder activation `name` as an NCHW device array (a converted copy when the encoder ran channel-blocked)."""
        a = self.act[name]
        names = [g[0] for g in self.enc_geom]
        if self.fp16_conv and name in names[:-1]:
            # the fp16 encoder wrote only the NHWC fp16 tensor: its values as NCHW fp32 (the fp32 decoder's skip inputs)
            lib.deepim_nhwc_f16_to_nchw_f32(self.ctx.handle, a, self.act[name + "_h"], a.shape[0], a.shape[1], a.shape[2], a.shape[3])
            return a
        if self.act_layout == "x3" and name in names[:-1]:
            lib.deepim_split16_to_nchw_f32(self.ctx.handle, a, self.act[name + "_x"], a.shape[0], a.shape[1], a.shape[2],
                                           a.shape[3], ctypes.c_float(1.0 / self.X3_ACT_SCALE))
            return a
        if self.fp16_conv or self.act_layout != "nc8" or name not in names[:-1]:
            return a
        key = name + "_nchw"          # one conversion buffer per tensor, allocated on first use (not during graph capture)
        if key not in self.act:
            self.act[key] = self.ctx.empty(a.shape)
        out = self.act[key]
        if self._enc_out_mode(names.index(name)) == 3:
            lib.deepim_relayout_nc8_s2d(self.ctx.handle, out, a, a.shape[0], a.shape[1], a.shape[2], a.shape[3], 0)
            return out
        lib.deepim_relayout_nc8(self.ctx.handle, out, a, a.shape[0], a.shape[1], a.shape[2] * a.shape[3], 0)
        return out

    FC6_PLAIN_MAX_BATCH = 4   # measured (tools/bench_fc6.py): B = 1 / 4 / 32 → plain 20 / 24 / 79 µs, packed MFMA 31 / 31 / 32 µs

    def _fc6(self, flat):
        """fc6 (81920 → 256): up to FC6_PLAIN_MAX_BATCH pairs the plain kernel streams the raw weights once faster than the MFMA
        kernel runs on the packed ones (and a training step then needs no 38 µs re-pack of 84 MB); larger batches take the packed
        MFMA path. Fixed by the batch size, so every rank and run sums in the same order."""
        A, P, h, B = self.act, self.params, self.ctx.handle, self.B
        if B <= self.FC6_PLAIN_MAX_BATCH:
            lib.deepim_fc_forward(h, A["fc6"], flat, P["fc6_weight"], P["fc6_bias"], B, flat.shape[1], 256, ctypes.c_float(SLOPE))
        else:
            lib.deepim_fc_forward_packed(h, A["fc6"], flat, self.packed["fc6"], P["fc6_bias"], B, flat.shape[1], 256,
                                         ctypes.c_float(SLOPE))

    def pose_head(self):
        A, P, h, B = self.act, self.params, self.ctx.handle, self.B
        flat = A["conv6_1"].reshape((B, -1))
        self._fc6(flat)
        lib.deepim_fc_forward(h, A["fc7"], A["fc6"], P["fc7_weight"], P["fc7_bias"], B, 256, 256,
                              ctypes.c_float(SLOPE))
        if self.rot_type == "EULER":      # 3-output rot head (deepIM_flownet.py:715-726): FullyConnected x2, inverse ZoomTrans, Concat
            c1 = ctypes.c_float(1.0)
            lib.deepim_fc_forward(h, A["rot_e"], A["fc7"], P["rot_weight"], P["rot_bias"], B, 256, 3, c1)
            lib.deepim_fc_forward(h, A["zoom_trans_e"], A["fc7"], P["trans_weight"], P["trans_bias"], B, 256, 3, c1)
            lib.deepim_zoom_trans_forward(h, A["zoom_factor"], A["zoom_trans_e"], A["trans_e"], 1, B)
            lib.deepim_copy_channels(h, A["se3"], 6, 0, A["rot_e"], 3, B, 1)
            lib.deepim_copy_channels(h, A["se3"], 6, 3, A["trans_e"], 3, B, 1)
            return
        lib.deepim_pose_head_forward(h, A["se3"], A["fc7"], P["rot_weight"], P["rot_bias"], P["trans_weight"],
                                     P["trans_bias"], A["zoom_factor"], B, 256)

    def pose_head_update(self, src_pose, pose_out=None):
        """pose_head() + pose_update() with everything behind fc6 in ONE launch (deepim_pose_tail_forward: fc7 → rot / trans +
        inverse ZoomTrans → se3 → RT_transform); bit-identical to the separate calls, fills the same activations (fc6, fc7,
        se3) and returns the refined poses. `pose_out` may be `src_pose` (in-place update, as the refinement loop does)."""
        A, P, h, B = self.act, self.params, self.ctx.handle, self.B
        out = A["pose_est"] if pose_out is None else pose_out
        if self.rot_type == "EULER":      # the fused tail is the quaternion form; EULER takes the separate launches
            self.pose_head()
            return self.pose_update(src_pose, out)
        self._fc6(A["conv6_1"].reshape((B, -1)))
        lib.deepim_pose_tail_forward(h, A["fc7"], A["se3"], out, A["fc6"], P["fc7_weight"], P["fc7_bias"], P["rot_weight"],
                                     P["rot_bias"], P["trans_weight"], P["trans_bias"], A["zoom_factor"], src_pose, self.T_means,
                                     self.T_stds, self.rot_coord, B, 256, ctypes.c_float(SLOPE))
        return out

    def _skip_into(self, cat):
        """Concat's first input: its encoder activation into channels [0, C) of the concat tensor — straight from the channel-blocked
        tensor where the encoder ran channel-blocked (one pass instead of relayout + 2-D blit), else a slice copy."""
        A, h, B = self.act, self.ctx.handle, self.B
        ctotal, (ho, wo), name, C = CONCAT[cat]
        names = [g[0] for g in self.enc_geom]
        if self.act_layout == "nc8" and not self.fp16_conv and name in names[:-1]:
            if self._enc_out_mode(names.index(name)) == 3:   # written space-to-depth for the stride-2 layer after it
                a = A[name]
                lib.deepim_relayout_nc8_s2d_slice(h, A[cat], ctotal, 0, a, B, C, a.shape[2], a.shape[3])
            else:
                lib.deepim_relayout_nc8_slice(h, A[cat], ctotal, 0, A[name], B, C, ho * wo)
        else:
            lib.deepim_copy_channels(h, A[cat], ctotal, 0, self.activation_nchw(name), C, B, ho * wo)

    def decoder(self):
        """FlowNetS refinement (deepIM_flownet.py:120-167): Concat2 = [conv5_1 | lrelu(deconv5) | upsample_flow6to5], Concat3 =
        [conv4_1 | lrelu(deconv4) | upsample_flow5to4]. fp16 decoder: the concats NHWC fp16 (zero-padded), flow6 / flow5 fp32 NCHW."""
        A = self.act
        if self.fp16_decoder:
            self._fewout16("Convolution1", ["Convolution1"], A["conv6_1_h"])
            self._concat16("Concat2", A["conv6_1_h"], "flow6")
            self._fewout16("Convolution2", ["Convolution2"], A["Concat2_h"])
            return self._concat16("Concat3", A["Concat2_h"], "flow5")
        self._pred("Convolution1", A["conv6_1"])
        self._skip_into("Concat2")
        self._deconv("deconv5", A["conv6_1"])
        self._deconv("upsample_flow6to5", A["flow6"])
        self._pred("Convolution2", A["Concat2"])
        self._skip_into("Concat3")
        self._deconv("deconv4", A["Concat2"])
        self._deconv("upsample_flow5to4", A["flow5"])

    def _upsample16(self, name, scale):
        """The fixed bilinear 16x upsampling + Crop `name` of DECODER from its low-resolution predictor's output."""
        l = DECODER[name]
        src = next(p.out for p in DECODER.values() if p.kind == "pred" and p.head == l.head)
        lib.deepim_upsample16_crop_forward(self.ctx.handle, self.act[l.out], self.act[src], self.params[name + "_weight"], self.B, l.cout,
                                           l.hw_in[0], l.hw_in[1], self.H, self.W, 8, 8, ctypes.c_float(scale))

    def heads(self):
        A, h, B, H, W = self.act, self.ctx.handle, self.B, self.H, self.W
        # both predictors stream the same 770-channel Concat3: back to back, so that the second finds it where the first left it (the
        # Infinity Cache) instead of behind the 120 MB the first head's upsampling + inverse zoom move (round 6 trace: 62 -> 40 us at B = 32)
        if self.fp16_decoder:   # fp16 Concat3: both predictors in ONE pass over it
            self._fewout16("heads", self.heads16, A["Concat3_h"])
        else:                   # mask_conv3 (deepIM_flownet.py:627-666), then Convolution3 (:677-713)
            for name in self.heads16:
                self._pred(name, A["Concat3"])
        if self.with_mask_head:
            self._upsample16("mask_upsampling", 1.0)
            lib.deepim_mask_head_forward(h, A["mask_observed_pred"], None, A["mask_logits"], A["zoom_factor"], B, H, W)
        if self.with_flow_head:
            self._upsample16("upsampling", self.normalize_flow)
            lib.deepim_zoom_flow_forward(h, A["zoom_factor"], A["zoom_flow_est"], None, A["flow_est"], None, 1, B, H, W)

    def pose_update(self, src_pose, pose_out=None):
        """RT_transform of every pair (tester.py:391-398)."""
        out = self.act["pose_est"] if pose_out is None else pose_out
        fn = lib.deepim_rt_transform_euler if self.rot_type == "EULER" else lib.deepim_rt_transform   # RT_transform.py:138-143
        fn(self.ctx.handle, out, None, src_pose, self.act["se3"], self.T_means, self.T_stds, self.rot_coord, self.B)
        return out

    def forward(self, data):
        """One network forward = `Predictor.predict` (tester.py:45-47). Returns the output dict (device arrays)."""
        self._trunk(data)
        self.pose_head()
        out = {"se3": self.act["se3"], "zoom_factor": self.act["zoom_factor"]}
        if self.with_mask_head:
            out["mask_observed_pred"] = self.act["mask_observed_pred"]
        if self.with_flow_head:
            out["flow_est_crop"] = self.act["flow_est"]
        return out

    def capture_iteration(self, data, pose_out=None):
        """Record one refinement iteration (all its launches) into a hipGraph and return the graph id. The
        buffers of `data` / `pose_out` are baked in: refresh their CONTENTS between replays, not the objects.
        Run `refine_iteration` once eagerly first (tap tables, split-K autotuning, scratch growth)."""
        gid = ctypes.c_int(-1)
        lib.deepim_graph_begin(self.ctx.handle)
        try:
            self.refine_iteration(data, pose_out)
        finally:
            lib.deepim_graph_end(self.ctx.handle, ctypes.byref(gid))
        return gid.value

    def replay(self, graph_id):
        lib.deepim_graph_launch(self.ctx.handle, graph_id)

    def refine_iteration(self, data, pose_out=None):
        """One pose-refinement iteration for the bound batch: zoom → network → inverse ZoomTrans →
        RT_transform.  `data["src_pose"]` is the current estimate; returns the refined (B,3,4) poses."""
        self._trunk(data)
        return self.pose_head_update(data["src_pose"], pose_out)

    def _trunk(self, data):
        self.zoom(data)
        self.encoder()
        if self.with_decoder:
            self.decoder()
            self.heads()


"""Training side of the FlowNetS matching network (symbols/deepIM_flownet.py): bind_train, forward_train, backward, update and
train_step as a mixin of deepIM_flownet. Everything here runs on the buffers and the forward pieces of that class."""
from __future__ import annotations

import ctypes

import numpy as np

from ..runtime import Context, lib
from .deepIM_flownet import CONCAT, DECODER, ENCODER, FC6_IN, SLOPE, _out_hw


class _Grads(dict):
    """name → gradient in the parameter's own layout. The conv / deconv weight gradients that the LDS-staged kernel leaves
    tap-major (`tm`: name → (raw (Cout,kh*kw,Cin) buffer, Cout, Cin, kh*kw), deepim_conv2d_wgrad_tm) are permuted into the stored
    natural buffer when somebody asks for them; the SGD kernel reads the raw buffers in place, so a training step never does."""

    def __init__(self, ctx, *a, **kw):
        super().__init__(*a, **kw)
        self._ctx, self.tm = ctx, {}

    def __getitem__(self, name):
        out = dict.__getitem__(self, name)
        if name in self.tm:
            raw, cout, cin, khw = self.tm[name]
            lib.deepim_weight_grad_to_natural(self._ctx.handle, out, raw, cout, cin, khw)
        return out

    def items(self):
        return [(k, self[k]) for k in self]

    def values(self):
        return [self[k] for k in self]


class TrainGraph(object):
    """bind_train / forward_train / backward / update / train_step of deepIM_flownet (its mixin)."""

    def bind_train(self, ctx, batch_size, arg_params, num_points=3000):
        """bind() + gradient, momentum and workspace buffers for one training-style iteration."""
        assert self.is_train, "call get_symbol(cfg, is_train=True) first"
        self.bind(ctx, batch_size, arg_params)
        B, H, W = self.B, self.H, self.W
        # rot / trans FullyConnected run their backward as ONE 7-row layer: their weights and gradients live as row ranges of
        # shared (7,256) / (7,) buffers, so nothing is assembled or split per step
        self.side = Context(ctx.device_id) if self.two_streams else None     # second stream of the backward (see backward())
        w7, dw7, db7 = ctx.empty((7, 256)), ctx.zeros((7, 256)), ctx.zeros((7,))
        w7[0:4].copyfrom(self.params["rot_weight"]); w7[4:7].copyfrom(self.params["trans_weight"])
        self.params["rot_weight"], self.params["trans_weight"] = w7[0:4], w7[4:7]
        self.grad = _Grads(ctx, {name: ctx.zeros(a.shape) for name, a in self.params.items()})
        self._upd_ws = None        # train_step's batch-updater workspace is sized for the bound batch
        self._sgd_table = self._adam_table = None     # their rows hold raw pointers of the buffers allocated here: never reuse one across binds
        # tap-major weight gradients (deepim_conv2d_wgrad_tm) only where that entry applies: Cin % 8 == 0 and the LDS-staged
        # kernel selected on this context. Everything else (conv1 of the 6- / 10-channel inputs, wgrad_lds = 0) takes
        # deepim_conv2d_wgrad into the natural buffer and the SGD table reads that one (layout word 0).
        big_deconvs = (DECODER["deconv4"], DECODER["deconv5"])
        opt = ctypes.c_int(0)
        lib.deepim_get_option(ctx.handle, b"wgrad_lds", ctypes.byref(opt))
        if self.train_winograd and not opt.value:
            raise NotImplementedError("TRAIN.WINOGRAD_CONV needs the LDS-staged weight gradient (context option wgrad_lds = 1): the "
                                      "register-fed kernel reads NCHW activations only")
        for gname, cin, _h, _w, cout, k, _s, _p in self.enc_geom:       # conv layers: (Cout, Cin, k, k)
            if opt.value and cin % 8 == 0:
                self.grad.tm[gname + "_weight"] = (ctx.zeros((cout, k * k, cin)), cout, cin, k * k)
        if self.with_decoder and opt.value:                              # deconvs: MXNet (cin, cout, 4, 4) = filters cin, channels cout
            for l in big_deconvs:
                self.grad.tm[l.name + "_weight"] = (ctx.zeros((l.cin, 16, l.cout)), l.cin, l.cout, 16)
        self.grad["rot_weight"], self.grad["trans_weight"] = dw7[0:4], dw7[4:7]
        self.grad["rot_bias"], self.grad["trans_bias"] = db7[0:4], db7[4:7]
        # optimizer state, zero after every bind: SGD momenta, or Adam's two moments and the device step count (deepim_adam_update_multi)
        adam = self.optimizer == "adam"
        self.mom = {} if adam else {name: ctx.zeros(a.shape) for name, a in self.params.items()}
        self.adam_mean = {name: ctx.zeros(a.shape) for name, a in self.params.items()} if adam else {}
        self.adam_var = {name: ctx.zeros(a.shape) for name, a in self.params.items()} if adam else {}
        self.opt_state = ctx.zeros((4,), dtype=np.uint32) if adam else None      # {uint t, float lr_t, float lr_factor, 0}
        A = self.act
        A["rot"], A["rot_norm"] = ctx.empty((B, 4)), ctx.empty((B, 4))
        A["zoom_trans"], A["trans_est"] = ctx.empty((B, 3)), ctx.empty((B, 3))
        A["points_est"] = ctx.empty((B, 3, num_points))
        A["pm_loss"], A["pm_loss_sum"] = ctx.empty((B, 3, num_points)), ctx.empty((1,))
        self.num_points = num_points
        # backward workspaces: two ping-pong activation-gradient buffers, the un-cropped gradient of the decoder's transposed
        # convolutions, and the packed data-gradient weights (sized for the largest layer)
        big = max(int(np.prod(A[g[0]].shape)) for g in self.enc_geom)
        self.ws = {"ga": ctx.empty((big,)), "gb": ctx.empty((big,))}
        dil, pmax = 4, 4
        psize = lib.load().deepim_conv_packed_size
        for name, cin, h, w, cout, k, s_, p_ in self.enc_geom[1:]:
            pmax = max(pmax, psize(cin, cout, k, k) // 4)
            pmax = max(pmax, lib.load().deepim_conv_dgrad_packed_size(cout, cin, k, s_, p_) // 4)
        if self.with_decoder:
            # the un-cropped gradients of the two big transposed convolutions, and the role-swapped weights of the decoder layers
            dil = max([dil] + [B * l.cout * (2 * l.hw_in[0] + 2) * (2 * l.hw_in[1] + 2) for l in big_deconvs])
            pmax = max([pmax] + [psize(l.cin, l.cout, 4, 4) // 4 for l in big_deconvs]
                       + [psize(l.cin, l.cout, 3, 3) // 4 for l in (DECODER["Convolution2"], DECODER["Convolution3"])])
            W_ = self.ws
            for cat, d_skip in (("Concat3", "d_skip4"), ("Concat2", "d_skip5")):
                ctotal, hw, _skip, cskip = CONCAT[cat]
                W_["d_" + cat], W_[d_skip] = ctx.empty((B, ctotal) + hw), ctx.empty((B, cskip) + hw)
            W_["d_dec61"] = ctx.empty(A["conv6_1"].shape)
            W_["d_flow5"], W_["d_flow6"] = ctx.empty(A["flow5"].shape), ctx.empty(A["flow6"].shape)
            W_["d_low"] = ctx.empty((B, 2) + DECODER["Convolution3"].hw_out)
        if self.with_flow_head:
            A["flow_loss"], A["flow_loss_sum"] = ctx.empty((B, 2, H, W)), ctx.empty((1,))
            A["zoom_flow_gt"], A["zoom_flow_weights"] = ctx.empty((B, 2, H, W)), ctx.empty((B, 2, H, W))
            self.ws["d_flow_hi"] = ctx.empty((B, 2, H, W))
        if self.with_mask_head:
            A["mask_prob"], A["zoom_mask_gt_observed"] = ctx.empty((B, 1, H, W)), ctx.empty((B, 1, H, W))
            self.ws["zm_a"], self.ws["zm_b"], self.ws["zm_f"] = ctx.empty((B, 1, H, W)), ctx.empty((B, 1, H, W)), ctx.empty((B, 4))
            self.ws["d_mask_hi"] = ctx.empty((B, 1, H, W))
        self.ws["dil"], self.ws["wt_packed"] = ctx.empty((dil,)), ctx.empty((pmax,))
        if self.train_winograd:
            # the 3x3 stride-1 data gradients on the Winograd kernels: U' per layer, and ONE channel-blocked dz buffer (the largest
            # such layer's output) that the activation-gradient walk fills next to the NCHW dz
            self._pack_wino_dgrad(True)
            if self.packed_wino_dgrad:
                self.ws["dz_nc8"] = ctx.empty((max(A[name].size for name in self.packed_wino_dgrad),))
        self.ws["g256a"], self.ws["g256b"] = ctx.empty((B, 256)), ctx.empty((B, 256))
        self.ws["dy7"], self.ws["w7"], self.ws["dw7"], self.ws["db7"] = ctx.empty((B, 7)), w7, dw7, db7
        self.ws["d_points"] = ctx.empty((B, 3, num_points))
        self.ws["d_rot_norm"], self.ws["d_trans_est"] = ctx.empty((B, 4)), ctx.empty((B, 3))
        self.ws["d_rot"], self.ws["d_trans"] = ctx.empty((B, 4)), ctx.empty((B, 3))
        if self.fp16_conv or self.train_x3:
            self._bind_train_half()
        if self.se3_dist_loss:            # deepIM_flownet.py:238-262
            A["zoom_trans_gt"], A["rot_loss"] = ctx.empty((B, 3)), ctx.empty((B,))
            A["trans_loss"], A["trans_loss_sum"] = ctx.empty((B, 3, 1)), ctx.empty((1,))
            self.ws["d_rot_norm_dist"], self.ws["d_zoom_trans_dist"] = ctx.empty((B, 4)), ctx.empty((B, 3, 1))
        ctx.sync()
        return self

    def _bind_train_half(self):
        """Buffers of the half-precision encoder backward, fp16 or split-fp16 (for x3 bind() already made packed_x3, conv1's pack
        included, and the split16 activations): two gradient buffers in the mode's layout (ping-pong, sized for the largest
        activation), the dgrad workspace (packed weights + parity-class buffer), and the scale state {scale, inv_scale, overflow,
        good_steps}."""
        ctx, B, x3 = self.ctx, self.B, self.train_x3
        if x3 and ENCODER[0][0] not in self.packed_x3:
            raise NotImplementedError("TRAIN.X3_CONV needs the 8-channel network input with W % 4 == 0 (conv1 on the split-fp16 patch "
                                      "kernel)")
        ga, gb, gws = ("gx3a", "gx3b", "dgradx3") if x3 else ("g16a", "g16b", "dgrad16")
        halves = 2 if x3 else 1      # fp16 words per element: a split16 tensor carries hi and lo
        big = max(self.act[g[0]].size for g in self.enc_geom)
        self.ws[ga] = ctx.empty((halves * big,), dtype=np.float16)
        self.ws[gb] = ctx.empty((halves * big,), dtype=np.float16)
        L = lib.load()
        ws_size = L.deepim_conv_dgrad_x3_workspace_size if x3 else L.deepim_conv_dgrad_f16_workspace_size
        nb = max(ws_size(B, cin, hh, ww, cout, k, s_, p_)      # (x3: conv2's data gradient, Cin = 64, runs on the fp32 kernels)
                 for _n, cin, hh, ww, cout, k, s_, p_ in self.enc_geom[1:] if not x3 or cin % 128 == 0)
        self.ws[gws] = ctx.empty(((nb + 1) // 2,), dtype=np.float16)
        self.amp_state = ctx.empty((4,), dtype=np.uint32)
        self.set_loss_scale(self.loss_scale_init)

    def set_loss_scale(self, scale, good_steps=0):
        """Overwrite the device loss-scale state: scale (a power of two), overflow cleared."""
        v = self._check_loss_scale(scale)
        st = np.zeros(4, np.uint32)
        st[:2] = np.array([v, 1.0 / v], np.float32).view(np.uint32)
        st[3] = int(good_steps)
        self.amp_state.copyfrom(st)

    def loss_scale(self):
        """The device loss-scale state as a dict (for logging and tests). The only call of the fp16 / x3 training graphs that syncs."""
        st = self.amp_state.asnumpy()
        f = st[:2].view(np.float32)
        return {"scale": float(f[0]), "inv_scale": float(f[1]), "overflow": bool(st[2]), "good_steps": int(st[3])}

    def _encoder_backward_half(self, e61):
        """Backward of the half-precision encoder, last layer first, one loop for both modes (csrc/train_half.hip). e61: the fp32
        NCHW gradient reaching conv6_1 (fc6 data gradient + d_dec61), scaled by S inside the first walk.
        fp16: dz = q(lrelu'(y)·e) and db in one walk, dW on the fp16 matrix cores, d = q(conv_transpose(dz,
        q(w))) into the other NHWC fp16 buffer.
        x3: dz = split(lrelu'(y)·e, 1) and db in one walk, dW as three fp16 MFMAs per fragment pair, d =
        split(conv_transpose(dz, split(w, s_w)) / s_w, 1) into the other split16 buffer. The two shapes the x3 kernels do not take
        run on the fp32 kernels over converted tensors: conv1's weight gradient (Cin = 8) and conv2's data gradient (64 output
        channels); the fp32 ping-pong buffers are free for them once the first walk has read e61."""
        A, P, G, W_, h, B = self.act, self.params, self.grad, self.ws, self.ctx.handle, self.B
        c, st, x3 = ctypes.c_float, self.amp_state, self.train_x3
        skips = {"conv5_1": W_["d_skip5"], "conv4_1": W_["d_skip4"]} if self.with_decoder else {}
        if x3:
            lib.deepim_x3_status_to_state(h, st)      # a clamp in the forward: the step is skipped, as after one in the backward
            x_, y_, sfx = W_["gx3a"], W_["gx3b"], "_x"
            fa, fb = W_["ga"], W_["gb"]
            lrelu_bias_backward = lib.deepim_lrelu_bias_backward_x3
        else:
            x_, y_, sfx = W_["g16a"], W_["g16b"], "_h"
            lrelu_bias_backward = lib.deepim_lrelu_bias_backward_f16
        for li in range(len(self.enc_geom) - 1, -1, -1):
            name, cin_, hh_, ww_, cout_, k_, s_, p_ = self.enc_geom[li]
            ho_, wo_ = _out_hw(hh_, ww_, k_, s_, p_)
            last = li == len(self.enc_geom) - 1
            lrelu_bias_backward(h, x_, G[name + "_bias"], None if last else x_, e61 if last else skips.get(name), A[name + sfx], st,
                                c(SLOPE), B, cout_, ho_, wo_)
            tm = G.tm.get(name + "_weight")
            dw, layout = (tm[0], 1) if tm else (dict.__getitem__(G, name + "_weight"), 0)
            if x3 and li == 0:      # dz in real units as NCHW fp32, then the fp32 weight gradient from the NCHW net input
                lib.deepim_split16_to_nchw_f32_unscaled(h, fa, x_, st, B, cout_, ho_, wo_, c(1.0))
                wgrad = lib.deepim_conv2d_wgrad_tm if layout else lib.deepim_conv2d_wgrad
                wgrad(h, dw, A["net_input"], fa, B, cin_, hh_, ww_, cout_, k_, k_, s_, p_)
                break
            if x3:
                lib.deepim_conv2d_wgrad_x3(h, dw, A[self.enc_geom[li - 1][0] + "_x"], x_, st, B, cin_, hh_, ww_, cout_, k_, s_, p_,
                                           layout, c(self.X3_ACT_SCALE))
            else:
                cpad = (cin_ + 7) // 8 * 8
                if li == 0:      # conv1's input as NHWC fp16 (the training zoom wrote NCHW fp32)
                    lib.deepim_nchw_f32_to_nhwc_f16(h, A["net_input_h"], A["net_input"], B, cin_, hh_, ww_, cpad)
                    src = A["net_input_h"]
                else:
                    src = A[self.enc_geom[li - 1][0] + "_h"]
                lib.deepim_conv2d_wgrad_f16(h, dw, src, x_, st, B, cin_, cpad, hh_, ww_, cout_, k_, s_, p_, layout)
            if li == 0:          # no data gradient below conv1 (x3 has left the loop there already)
                break
            if x3:
                if cin_ % 128 == 0:
                    lib.deepim_conv2d_dgrad_x3(h, y_, x_, P[name + "_weight"], W_["dgradx3"], st, B, cin_, hh_, ww_, cout_, k_, s_, p_,
                                               c(self.x3_wscale[name]))
                else:            # conv2: the scaled dz as NCHW fp32 → fp32 data gradient → split16 at scale 1
                    lib.deepim_split16_to_nchw_f32(h, fa, x_, B, cout_, ho_, wo_, c(1.0))
                    self._dgrad(fb, fa, P[name + "_weight"], B, cin_, hh_, ww_, cout_, k_, s_, p_, ho_, wo_)
                    lib.deepim_nchw_f32_to_split16(h, y_, fb, B, cin_, hh_, ww_, c(1.0))
                    lib.deepim_x3_status_to_state(h, st)
            else:
                lib.deepim_conv2d_dgrad_f16(h, y_, x_, P[name + "_weight"], W_["dgrad16"], B, cin_, hh_, ww_, cout_, k_, s_, p_)
            x_, y_ = y_, x_
        return G

    def forward_train(self, data, label):
        """data: image_observed, image_rendered, mask_observed, mask_rendered [, depth_*], src_pose; label:
        mask_gt_observed, point_cloud_model, point_cloud_weights, point_cloud_observed [, flow, flow_weights] (device arrays).
        Returns the point-matching loss sum (device scalar) after filling every activation the backward needs; the flow loss
        and the mask probability land in self.act["flow_loss"] / ["mask_prob"]."""
        if data.get("observed_frames") is not None:
            raise NotImplementedError("forward_train: a shared-frame batch (data['observed_frames']) is a test-phase input; the "
                                      "training graph reads per-pair image_observed tensors")
        A, P, h, B, H, W = self.act, self.params, self.ctx.handle, self.B, self.H, self.W
        c = ctypes.c_float
        t = self.cfg.train_iter
        lib.deepim_zoom_concat_train_forward(
            h, data["image_observed"], data["image_rendered"], data["mask_observed"] if self.input_mask else None,
            label["mask_gt_observed"] if self.input_mask else None, data["mask_rendered"] if self.input_mask else None,
            data.get("depth_observed") if self.input_depth else None, data.get("depth_rendered") if self.input_depth else None,
            data["src_pose"], self.K, self.pixel_means, A["net_input"], A["zoom_factor"], B, H, W)
        self.encoder()
        if self.with_decoder:
            self.decoder()
        if self.with_flow_head:   # deepIM_flownet.py:183-207 (+ the ZoomFlow of the labels, :478-492)
            self._pred("Convolution3", A["Concat3"])
            self._upsample16("upsampling", 1.0)                      # flow_est_crop, in units of NORMALIZE_FLOW
            lib.deepim_zoom_flow_forward(h, A["zoom_factor"], label["flow"], label["flow_weights"], A["zoom_flow_gt"],
                                         A["zoom_flow_weights"], 0, B, H, W)
            lib.deepim_flow_loss(h, A["flow_loss"], A["flow_loss_sum"], self.ws["d_flow_hi"], A["zoom_flow_est"],
                                 A["zoom_flow_gt"], A["zoom_flow_weights"], c(self.normalize_flow), c(t.LW_FLOW / (480 * 640)),
                                 B * 2 * H * W)
        if self.with_mask_head:   # :314-361 (+ ZoomMask of mask_gt_observed, :395-412)
            self._pred("mask_conv3", A["Concat3"])
            self._upsample16("mask_upsampling", 1.0)
            lib.deepim_zoom_mask_forward(h, data["mask_observed"], label["mask_gt_observed"], data["mask_rendered"],
                                         data["src_pose"], self.K, self.ws["zm_a"], A["zoom_mask_gt_observed"], self.ws["zm_b"],
                                         self.ws["zm_f"], B, H, W)
            # LogisticRegressionOutput: grad = grad_scale / num_output · (p − y), num_output = H·W per sample
            lib.deepim_mask_logistic(h, A["mask_prob"], self.ws["d_mask_hi"], A["mask_logits"], A["zoom_mask_gt_observed"],
                                     c(t.LW_MASK / (H * W)), B * H * W)
        flat = A["conv6_1"].reshape((B, -1))
        self._fc6(flat)
        lib.deepim_fc_forward(h, A["fc7"], A["fc6"], P["fc7_weight"], P["fc7_bias"], B, 256, 256, c(SLOPE))
        lib.deepim_fc_forward(h, A["rot"], A["fc7"], P["rot_weight"], P["rot_bias"], B, 256, 4, c(1.0))
        lib.deepim_fc_forward(h, A["zoom_trans"], A["fc7"], P["trans_weight"], P["trans_bias"], B, 256, 3, c(1.0))
        lib.deepim_l2_normalize_forward(h, A["rot_norm"], A["rot"], B, 4, c(1e-10))                       # :217
        lib.deepim_zoom_trans_forward(h, A["zoom_factor"], A["zoom_trans"], A["trans_est"], 1, B)           # :218-225
        ltypes = {"L1": 0, "L2": 1, "smooth_L1": 2}
        if self.se3_dist_loss:            # :238-262: rot_loss = 1 - (q_gt . q_est)^2 (grad_scale LW_ROT), trans loss on the ZOOMED deltas
            rot_gt = label["rot"] if "rot" in label else label["rot_gt"]            # Variable(name="rot") / ("trans"), :452-453
            trans_gt = label["trans"] if "trans" in label else label["trans_gt"]
            lib.deepim_zoom_trans_forward(h, A["zoom_factor"], trans_gt, A["zoom_trans_gt"], 0, B)         # :455-457
            lib.deepim_rot_dist_loss(h, A["rot_loss"], self.ws["d_rot_norm_dist"], rot_gt, A["rot_norm"], c(t.LW_ROT), B)
            lib.deepim_point_matching_loss(h, A["trans_loss"], A["trans_loss_sum"], self.ws["d_zoom_trans_dist"], A["zoom_trans"],
                                           A["zoom_trans_gt"], None, c(1.0), ltypes[self.trans_loss_type],
                                           c(t.get("TRANS_SMOOTH_L1_SCALAR", 3.0)), c(t.LW_TRANS), B, 1)
        if self.se3_pm_loss:
            lib.deepim_transform3d_forward(h, A["points_est"], label["point_cloud_model"], A["rot_norm"], A["trans_est"],
                                           data["src_pose"], self.T_means, self.T_stds, self.rot_coord, B, self.num_points)
            lib.deepim_point_matching_loss(h, A["pm_loss"], A["pm_loss_sum"], self.ws["d_points"], A["points_est"],
                                           label["point_cloud_observed"], label["point_cloud_weights"],
                                           c(self.cfg.dataset.NORMALIZE_3D_POINT), ltypes[t.SE3_PM_LOSS_TYPE], c(t.SE3_PM_SL1_SCALAR),
                                           c(t.LW_PM / t.NUM_3D_SAMPLE), B, self.num_points)                    # :265-312
        self._train_io = (data, label)
        return A["pm_loss_sum"] if self.se3_pm_loss else A["trans_loss_sum"]

    def _dgrad(self, dx, dz, w_raw, B, cin, hh, ww, cout, k, s_, p_, ho, wo, act_y=None, add=None):
        """dx (B,cin,hh,ww) of a Convolution (cout,cin,k,k; stride s_, pad p_) given dz (B,cout,ho,wo); with act_y (the saved output
        of the layer below, [+ add: the gradient arriving over its skip connection]) dx already is that layer's dz =
        lrelu'(act_y)·(dx + add), applied in the convolution's final stores.
        stride 1: the forward MFMA conv kernel on dz with the transposed, flipped weights, pad k-1-p.
        stride 2: four stride-1 convolutions of the UN-dilated dz, one per output parity class (y % 2, x % 2) with the
        sub-kernel of the taps that class meets (k = 3: 1, 2, 2 and 4 taps; k = 5: 4, 6, 6 and 9), each storing its result
        window on its parity positions of dx — exactly the ideal multiply-adds (round 2 convolved a zero-dilated dz: 4x those);
        the four classes are packed, convolved and reduced by one launch each."""
        lib.deepim_conv2d_dgrad(self.ctx.handle, dx, dz, w_raw, self.ws["wt_packed"], B, cin, hh, ww, cout, k, s_, p_, act_y, add,
                                ctypes.c_float(SLOPE))

    def _small_conv_backward(self, name, src, dz, dx):
        """A 3x3 s1 p1 prediction layer of DECODER (Convolution1/2/3, mask_conv3): gradients into self.grad, data gradient into dx."""
        h, B, l = self.ctx.handle, self.B, DECODER[name]
        (hh, ww), cin, cout = l.hw_in, l.cin, l.cout
        lib.deepim_conv2d_wgrad_bias(h, self.grad[name + "_weight"], self.grad[name + "_bias"], src, dz, B, cin, hh, ww, cout, 3, 3, 1, 1)
        self._dgrad(dx, dz, self.params[name + "_weight"], B, cin, hh, ww, cout, 3, 1, 1, hh, ww)

    def _head_backward(self, up, name, d_hi, first):
        """A head on Concat3, bilinear upsampling `up` (fixed, lr_mult 0) → predictor `name` (Convolution3 / mask_conv3): the
        first head writes d_Concat3, the second adds to it."""
        W_, h, l = self.ws, self.ctx.handle, DECODER[up]
        lib.deepim_upsample16_crop_backward(h, W_["d_low"], d_hi, self.params[up + "_weight"], self.B, l.cout, l.hw_in[0], l.hw_in[1],
                                            self.H, self.W, 8, 8, ctypes.c_float(1.0))
        self._small_conv_backward(name, self.act["Concat3"], W_["d_low"], W_["d_Concat3"] if first else W_["ga"])
        if not first:
            lib.deepim_axpy(h, W_["d_Concat3"], W_["ga"], ctypes.c_float(1.0), W_["d_Concat3"].size)

    def _deconv_backward(self, name, x, dx):
        """Deconvolution k4 s2 + Crop(1,1) [+ LeakyReLU] of DECODER whose output is channels [coff, coff+cout) of a Concat, from the
        concat's gradient (B,ctotal,ho,wo) and, where the layer has an activation, the saved concat. Bias / weight gradients into
        self.grad, data gradient (B,cin,hh,ww) into dx. One walk slices the concat gradient, applies the activation gradient, sums
        the bias gradient and puts the result back into the un-cropped frame; the MXNet weight (cin,cout,4,4) already is the
        Convolution layout of the adjoint (filters = cin, channels = cout), so the data gradient is a stride-2 convolution of that
        frame and the weight gradient a conv wgrad with input and output swapped."""
        h, B, l = self.ctx.handle, self.B, DECODER[name]
        (hh, ww), (ho, wo), cin, cout = l.hw_in, l.hw_out, l.cin, l.cout
        hf, wf = 2 * hh + 2, 2 * ww + 2
        ycat = self.act[l.out] if l.slope != 1.0 else None
        lib.deepim_slice_lrelu_bias_scatter(h, self.ws["dil"], self.grad[name + "_bias"], self.ws["d_" + l.out], ycat, B, CONCAT[l.out][0],
                                            l.coff, cout, ho, wo, hf, wf, 1, 1, ctypes.c_float(SLOPE))
        if name + "_weight" in self.grad.tm:
            lib.deepim_conv2d_wgrad_tm(h, self.grad.tm[name + "_weight"][0], self.ws["dil"], x, B, cout, hf, wf, cin, 4, 4, 2, 0)
        else:
            lib.deepim_conv2d_wgrad(h, self.grad[name + "_weight"], self.ws["dil"], x, B, cout, hf, wf, cin, 4, 4, 2, 0)
        order = lib.load().deepim_conv_weight_order(h, B, cout, hf, wf, cin, 4, 4, 2, 0)         # packed for this one use
        lib.deepim_conv_pack_weights_ex(h, self.ws["wt_packed"], self.params[name + "_weight"], cin, cout, 4, 4, order)
        lib.deepim_conv2d_forward(h, dx, self.ws["dil"], self.ws["wt_packed"], None, B, cout, hf, wf, cin, 4, 4, 2, 0,
                                  ctypes.c_float(1.0), 0, 0)

    def _skip_backward(self, cat, d_skip):
        """The gradient over a Concat's skip connection: its first channels, the encoder activation's."""
        ctotal, (ho, wo), _skip, cskip = CONCAT[cat]
        lib.deepim_extract_channels(self.ctx.handle, self.ws[d_skip], self.ws["d_" + cat], ctotal, 0, cskip, self.B, ho * wo)

    def _decoder_backward(self):
        """Backward of the flow / mask heads and the refinement decoder (deepIM_flownet.py:120-167): leaves the skip
        gradients in d_skip4 / d_skip5 and the conv6_1 gradient in d_dec61."""
        A, W_, h, c = self.act, self.ws, self.ctx.handle, ctypes.c_float
        if self.with_flow_head:
            self._head_backward("upsampling", "Convolution3", W_["d_flow_hi"], first=True)
        if self.with_mask_head:
            self._head_backward("mask_upsampling", "mask_conv3", W_["d_mask_hi"], first=not self.with_flow_head)
        # Concat3 = [conv4_1 | lrelu(deconv4) | upsample_flow5to4]
        self._skip_backward("Concat3", "d_skip4")
        self._deconv_backward("deconv4", A["Concat2"], W_["d_Concat2"])
        self._deconv_backward("upsample_flow5to4", A["flow5"], W_["d_flow5"])
        self._small_conv_backward("Convolution2", A["Concat2"], W_["d_flow5"], W_["ga"])
        lib.deepim_axpy(h, W_["d_Concat2"], W_["ga"], c(1.0), W_["d_Concat2"].size)
        # Concat2 = [conv5_1 | lrelu(deconv5) | upsample_flow6to5]
        self._skip_backward("Concat2", "d_skip5")
        self._deconv_backward("deconv5", A["conv6_1"], W_["d_dec61"])
        self._deconv_backward("upsample_flow6to5", A["flow6"], W_["d_flow6"])
        self._small_conv_backward("Convolution1", A["conv6_1"], W_["d_flow6"], W_["ga"])
        lib.deepim_axpy(h, W_["d_dec61"], W_["ga"], c(1.0), W_["d_dec61"].size)

    def backward(self):
        """module.backward (deepim/core/module.py:1131-1137): fills self.grad for every parameter."""
        A, P, G, W_, h, B = self.act, self.params, self.grad, self.ws, self.ctx.handle, self.B
        c = ctypes.c_float
        data, label = self._train_io
        if self.with_decoder:
            self._decoder_backward()
        if self.se3_pm_loss:
            lib.deepim_transform3d_backward(h, W_["d_rot_norm"], W_["d_trans_est"], W_["d_points"], label["point_cloud_model"],
                                            A["rot_norm"], A["trans_est"], data["src_pose"], self.T_means, self.T_stds,
                                            self.rot_coord, B, self.num_points)
            if self.se3_dist_loss:        # both heads of the gradient meet at rot_est_norm (:217 -> :240, :300)
                lib.deepim_axpy(h, W_["d_rot_norm"], W_["d_rot_norm_dist"], c(1.0), B * 4)
        else:
            W_["d_rot_norm"].copyfrom(W_["d_rot_norm_dist"])
        lib.deepim_l2_normalize_backward(h, W_["d_rot"], W_["d_rot_norm"], A["rot"], B, 4, c(1e-10))
        if self.se3_pm_loss:
            lib.deepim_zoom_trans_backward(h, A["zoom_factor"], W_["d_trans_est"], W_["d_trans"], 1, 0, B)     # b_zoom_grad=False
            if self.se3_dist_loss:        # ... and at zoom_trans_est (:212 -> :218, :251)
                lib.deepim_axpy(h, W_["d_trans"], W_["d_zoom_trans_dist"], c(1.0), B * 3)
        else:
            W_["d_trans"].copyfrom(W_["d_zoom_trans_dist"].reshape((B, 3)))
        # rot / trans FullyConnected as one 7-row layer: dy7 = [d_rot | d_trans], w7 = [rot_weight; trans_weight]
        lib.deepim_copy_channels(h, W_["dy7"], 7, 0, W_["d_rot"], 4, B, 1)
        lib.deepim_copy_channels(h, W_["dy7"], 7, 4, W_["d_trans"], 3, B, 1)
        lib.deepim_fc_backward(h, W_["g256a"], W_["dw7"], W_["db7"], W_["dy7"], A["fc7"], W_["w7"], B, 256, 7)   # G[rot_*], G[trans_*] are its rows
        # fc7, fc6 (LeakyReLU gradient from the saved outputs)
        lib.deepim_lrelu_backward(h, W_["g256a"], W_["g256a"], A["fc7"], c(SLOPE), B * 256)
        lib.deepim_fc_backward(h, W_["g256b"], G["fc7_weight"], G["fc7_bias"], W_["g256a"], A["fc6"], P["fc7_weight"], B, 256, 256)
        lib.deepim_lrelu_backward(h, W_["g256b"], W_["g256b"], A["fc6"], c(SLOPE), B * 256)
        ga, gb = W_["ga"], W_["gb"]
        lib.deepim_fc_backward(h, ga, G["fc6_weight"], G["fc6_bias"], W_["g256b"], A["conv6_1"].reshape((B, FC6_IN)),
                               P["fc6_weight"], B, FC6_IN, 256)
        if self.fp16_conv or self.train_x3:
            if self.with_decoder:
                lib.deepim_axpy(h, ga, W_["d_dec61"], c(1.0), B * FC6_IN)
            return self._encoder_backward_half(ga)
        skips = {"conv5_1": "d_skip5", "conv4_1": "d_skip4"} if self.with_decoder else {}
        # encoder, last layer first: dz = lrelu'(y)·(dy [+ the gradient over the layer's skip connection]) and the bias gradient in
        # one fused walk, in place over dy; dx into the other buffer. (_dgrad can apply the activation gradient of the layer below
        # in the convolution's own final stores instead — measured slower, 4.56 → 4.63 ms: the scattered epilogue reads of the
        # saved output cost more than the streaming pass they replace. profiles/r03_train_backward.md)
        # The weight gradient of a layer runs on a SECOND stream (self.side: own context, own scratch) next to the data gradient:
        # both only read dz, and on conv4 … conv6_1 neither fills the chip through its pack → convolution → second-pass chain.
        # Ordering: side waits for dz; main waits for the previous layer's weight gradient before its data gradient overwrites
        # the buffer that one reads (the two gradient buffers ping-pong).
        extra = {"conv6_1": "d_dec61", **skips} if self.with_decoder else {}
        side = self.side.handle if self.side is not None else h
        for li in range(len(self.enc_geom) - 1, -1, -1):
            name, cin_, hh_, ww_, cout_, k_, s_, p_ = self.enc_geom[li]
            ho_, wo_ = _out_hw(hh_, ww_, k_, s_, p_)
            add_ = W_[extra[name]] if name in extra else None
            y_mode = self._enc_out_mode(li) if self.train_winograd else 0     # how forward_train left this layer's output
            wdg = self.packed_wino_dgrad.get(name) if (self.train_winograd and li > 0) else None
            if wdg is not None and not lib.load().deepim_conv_wino_preferred(h, B, cout_, hh_, ww_, cin_):
                wdg = None    # (asked again per call: a context switched to the canonical order after bind takes the direct kernel)
            if y_mode or wdg is not None:      # (conv6_1 wrote NCHW for fc6, y_mode 0: the same walk for its channel-blocked dz)
                lib.deepim_lrelu_bias_backward_nc8(h, ga, W_["dz_nc8"] if wdg is not None else None, G[name + "_bias"], ga, add_, A[name],
                                                   y_mode, c(SLOPE), B, cout_, ho_, wo_)
            else:
                lib.deepim_lrelu_bias_backward(h, ga, G[name + "_bias"], ga, add_, A[name], c(SLOPE), B, cout_, ho_ * wo_)
            lib.deepim_stream_wait(h, side)      # weight gradient of layer li+1 done: gb may be overwritten
            lib.deepim_stream_wait(side, h)      # dz of this layer ready
            src = A["net_input"] if li == 0 else A[self.enc_geom[li - 1][0]]
            x_mode = self._enc_out_mode(li - 1) if (self.train_winograd and li > 0) else 0
            if x_mode:      # the producer's channel-blocked output, read in place (bind_train: wgrad_lds is on, Cin % 8 == 0)
                lib.deepim_conv2d_wgrad_tm_nc8(side, G.tm[name + "_weight"][0], src, x_mode, ga, B, cin_, hh_, ww_, cout_, k_, k_, s_, p_)
            elif name + "_weight" in G.tm:
                lib.deepim_conv2d_wgrad_tm(side, G.tm[name + "_weight"][0], src, ga, B, cin_, hh_, ww_, cout_, k_, k_, s_, p_)   # tap-major: _Grads
            else:       # Cin % 8 != 0 (6- / 10-channel conv1) or wgrad_lds = 0: natural (Cout, Cin, k, k) gradient
                lib.deepim_conv2d_wgrad(side, dict.__getitem__(G, name + "_weight"), src, ga, B, cin_, hh_, ww_, cout_, k_, k_, s_, p_)
            if li > 0 and wdg is not None:
                lib.deepim_conv2d_wino_dgrad(h, gb, W_["dz_nc8"], wdg, B, cin_, hh_, ww_, cout_)
            elif li > 0:
                self._dgrad(gb, ga, P[name + "_weight"], B, cin_, hh_, ww_, cout_, k_, s_, p_, ho_, wo_)
            ga, gb = gb, ga
        lib.deepim_stream_wait(h, side)          # every gradient is in place when the main stream goes on (update)
        return G

    def _update_table(self, key, wd, states):
        """The device pointer table of the multi-tensor optimizer kernels, cached per bind and weight decay: rows {w, *states, g, n,
        wd bits | first block << 32, layout of g} (deepim_sgd_mom_update_multi / deepim_adam_update_multi). As mx.optimizer does when
        Module hands it the parameter names: weight decay only on `*_weight` (wd_mult 0 elsewhere), and the bilinear upsampling
        kernels get no row (attr lr_mult 0, deepIM_flownet.py:193,333,643,695). -> (wd, table, rows, blocks)"""
        tab = vars(self)[key]
        if tab is None or tab[0] != float(wd):
            rows, block = [], 0
            for name, w in self.params.items():
                if name.endswith("upsampling_weight"):
                    continue
                wd_n = wd if name.endswith("_weight") else 0.0
                wd_bits = int(np.array([wd_n], np.float32).view(np.uint32)[0])
                if name in self.grad.tm:       # tap-major gradient, read in place: layout word = Cin | kh*kw << 32
                    raw, _co, cin_l, khw = self.grad.tm[name]
                    g_ptr, layout = raw.ptr, cin_l | (khw << 32)
                else:
                    g_ptr, layout = dict.__getitem__(self.grad, name).ptr, 0
                rows.append([w.ptr] + [s[name].ptr for s in states] + [g_ptr, w.size, wd_bits | (block << 32), layout])
                block += (w.size + 1023) // 1024
            dev = self.ctx.empty((len(rows), 5 + len(states)), np.uint64)
            dev.copyfrom(np.array(rows, dtype=np.uint64))
            tab = (float(wd), dev, len(rows), block)
            vars(self)[key] = tab
        return tab

    def update(self, lr, wd=None, momentum=0.975, rescale_grad=1.0, clip_gradient=None, beta1=0.9, beta2=0.999, epsilon=1e-8):
        """The optimizer step on every parameter, then the re-pack of the conv / deconv / fc6 weights the forward kernels read.
        TRAIN.optimizer = "sgd": train.py:296-303, MXNet sgd_mom_update; wd defaults to 0.0005; beta1 / beta2 / epsilon are ignored.
        TRAIN.optimizer = "adam": train.py:260-294, MXNet 1.2 adam_update with the step count on the device (include/deepim_hip.h);
        wd defaults to 0 (MXNet's default: the reference passes only the learning rate) and `momentum` is ignored. mx.optimizer
        would fill in rescale_grad = 1 / batch_size for Adam (core/module.py:522-536): pass it, as train_step does. The reference's
        non-xavier Adam branch (train.py:282-294) passes no optimizer_params at all and so runs at MXNet's default lr 0.01 whatever
        TRAIN.lr says; this port follows the explicit branch (:261): `lr` is what the caller gives.
        Weight decay only on `*_weight`, the bilinear upsampling kernels stay fixed (_update_table)."""
        h = self.ctx.handle
        c = ctypes.c_float
        amp = self.amp_state if (self.fp16_conv or self.train_x3) else None
        if self.optimizer == "adam":
            tab = self._update_table("_adam_table", 0.0 if wd is None else wd, (self.adam_mean, self.adam_var))
            # scaled gradients (amp): no parameter, no moment and no step count moves on a step whose gradients overflowed
            lib.deepim_adam_update_multi(h, tab[1], tab[2], tab[3], self.opt_state, ctypes.c_double(lr), ctypes.c_double(beta1),
                                         ctypes.c_double(beta2), c(epsilon), c(rescale_grad), c(clip_gradient or 0.0), amp)
        else:
            tab = self._update_table("_sgd_table", 0.0005 if wd is None else wd, (self.mom,))
            if amp is not None:
                lib.deepim_sgd_mom_update_multi_amp(h, tab[1], tab[2], tab[3], c(lr), c(momentum), c(rescale_grad),
                                                    c(clip_gradient or 0.0), amp)
            else:
                lib.deepim_sgd_mom_update_multi(h, tab[1], tab[2], tab[3], c(lr), c(momentum), c(rescale_grad), c(clip_gradient or 0.0))
        if amp is not None:
            lib.deepim_amp_scale_update(h, amp, self.loss_scale_window)      # then the scale step
        # the weights in the forms this mode's forward and backward read, through the functions that packed them at bind
        if self.fp16_conv:
            self._pack_f16(False)
        elif self.train_x3:
            self._pack_x3(False)
        orders = self._train_pack_orders()
        enc = {g[0] for g in self.enc_geom} if (amp is not None or self.train_winograd) else ()
        for base in self._direct_layers():
            if base not in enc:        # the fp16 / x3 encoder reads packed_f16 / packed_x3 only, the channel-blocked one _pack_wino's forms
                self._pack_direct(base, False, orders.get(base, 3))
        if self.train_winograd:
            self._pack_wino(False)
            self._pack_wino_dgrad(False)
        if self.B > self.FC6_PLAIN_MAX_BATCH:      # small batches read fc6's raw weights (_fc6)
            self._pack_fc6(False)

    def train_step(self, data, label, updater, iters=None, lr=None, wd=None, momentum=None, on_iter=None):
        """ONE training step as the reference runs it (deepim/core/module.py:1131-1137 with network.TRAIN_ITER_SIZE = 4, yaml
        :57-58): for every refinement iteration forward_backward → preds (rot_est, trans_est) → update (optimizer step + re-pack), and between
        iterations `interBatchUpdater.forward(data_batch, preds)` (lib/pair_matching/batch_updater_py_multi.py:91-328): pose ←
        RT_transform(src_pose, preds), re-render at it, new rot / trans labels (calc_RT_delta), K·T + lib/flow_c flow labels and
        weights, mask_rendered = depth > 0.2 — all resident, nothing allocated inside the loop, no host round trip.
        data must also carry tgt_pose [, depth_gt_observed with PRED_FLOW, class_index]; `updater` = batchUpdaterPyMulti with a
        device render machine. `on_iter(it, data, label)` is called after each iteration's update (tests, timers).
        `lr` is a float, or a callable lr(it) giving the learning rate of iteration `it`'s update (core/module.py fit hands the
        scheduler's value per update, as mx.optimizer asks its lr_scheduler). Returns (data, label) of the last iteration."""
        t = self.cfg.TRAIN
        iters = int(iters or self.cfg.network.TRAIN_ITER_SIZE)
        lr = t.lr if lr is None else lr
        adam = self.optimizer == "adam"
        # the optimizer's defaults as the reference reaches them: SGD gets TRAIN.wd / TRAIN.momentum and rescale_grad 1 (train.py:297-303);
        # Adam gets only the learning rate (:261), so wd = 0 and mx.optimizer's rescale_grad = 1 / batch_size (core/module.py:522-536)
        wd = (0.0 if adam else t.wd) if wd is None else wd
        momentum = t.momentum if momentum is None else momentum
        rescale = 1.0 / self.B if adam else 1.0
        if self._upd_ws is None or self._upd_ws[0] is not updater:
            self._upd_ws = (updater, updater.workspace(self.ctx, self.B))
        A = self.act
        for it in range(iters):
            self.forward_train(data, label)
            self.backward()
            preds = {"rot_est": A["rot_norm"], "trans_est": A["trans_est"]}     # get_outputs() before update(), as :1133-1134
            self.update(lr(it) if callable(lr) else lr, wd, momentum, rescale_grad=rescale)
            if on_iter is not None:
                on_iter(it, data, label)
            if it != iters - 1:
                batch = dict(label)
                batch.update(data)
                new = updater.forward(batch, preds, self.cfg, out=self._upd_ws[1])
                data = {k: new[k] for k in data}
                label = {k: new[k] for k in label}
        return data, label

    def train_outputs(self):
        """The outputs of the last forward_train that the training metrics read (core/metric.py), under the reference's output
        names (deepim/core/metric.py:13-48): views of self.act, nothing is copied."""
        A, out = self.act, {}
        if self.with_flow_head:
            out["flow_loss"] = A["flow_loss"]
        if self.se3_dist_loss:
            out["rot_loss"], out["trans_loss"] = A["rot_loss"], A["trans_loss"]
        if self.se3_pm_loss:
            out["point_matching_loss"] = A["pm_loss"]
        if self.with_mask_head:
            out["mask_prob"], out["mask_gt"] = A["mask_prob"], A["zoom_mask_gt_observed"]
        return out

    def optimizer_states(self):
        """The optimizer's state as host arrays, the resume half of module_checkpoint(..., save_optimizer_states=True) (train.py:242):
        {"mom:<name>"} for SGD, {"mean:<name>", "var:<name>", "t"} for Adam (t: int64, shape (1,)). mx.nd.save / mx.nd.load carry the
        dict. MXNet pickles its updater into the .states file, so no file-format parity with the reference is claimed."""
        if self.optimizer == "adam":
            out = {"mean:" + k: v.asnumpy() for k, v in self.adam_mean.items()}
            out.update({"var:" + k: v.asnumpy() for k, v in self.adam_var.items()})
            out["t"] = np.array([int(self.opt_state.asnumpy()[0])], np.int64)
            return out
        return {"mom:" + k: v.asnumpy() for k, v in self.mom.items()}

    def load_optimizer_states(self, states):
        """Restore what optimizer_states() returned (of the same optimizer and graph) into the bound buffers."""
        groups = {"mean": self.adam_mean, "var": self.adam_var} if self.optimizer == "adam" else {"mom": self.mom}
        want = {g + ":" + k for g, d_ in groups.items() for k in d_} | ({"t"} if self.optimizer == "adam" else set())
        if set(states) != want:
            raise ValueError("load_optimizer_states: these are not the states of this net's TRAIN.optimizer = {!r} (missing {}, unknown {})"
                             .format(self.optimizer, sorted(want - set(states))[:3], sorted(set(states) - want)[:3]))
        for g, d_ in groups.items():
            for k, buf in d_.items():
                a = np.asarray(states[g + ":" + k], np.float32)
                if a.shape != buf.shape:
                    raise ValueError("load_optimizer_states: {}:{} has shape {}, bound {}".format(g, k, a.shape, buf.shape))
                buf.copyfrom(a)
        if self.optimizer == "adam":
            st = np.zeros(4, np.uint32)       # lr_t / lr_factor are recomputed from t by the next update
            st[0] = int(np.asarray(states["t"]).ravel()[0])
            self.opt_state.copyfrom(st)

    def _train_pack_orders(self):
        """layer → the ONE packed operand order its forward convolution reads in the training graph (NCHW activations,
        deepim_conv_weight_order): the per-step re-pack writes only that one."""
        order = lib.load().deepim_conv_weight_order      # evaluated per update: follows the context's conv options
        h, B = self.ctx.handle, self.B
        # (TRAIN.WINOGRAD_CONV: the encoder layers are re-packed by _pack_wino in the orders the channel-blocked forward reads)
        geo = {} if self.train_winograd else {g[0]: g[1:] for g in self.enc_geom}
        for l in (DECODER[n] for n in ("Convolution1", "Convolution2", "Convolution3", "mask_conv3")):
            geo[l.name] = (l.cin,) + l.hw_in + (l.cout, 3, 1, 1)
        return {n: order(h, B, cin, hh, ww, cout, k, k, s_, p_) for n, (cin, hh, ww, cout, k, s_, p_) in geo.items()}

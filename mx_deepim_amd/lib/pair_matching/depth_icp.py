"""Depth ICP on the device: refine object poses against the observed depth map (csrc/icp.hip).

The reference's evaluation has an ICP row (TEST.PRECOMPUTED_ICP / TEST.BEFORE_ICP, deepim/core/tester.py:193-279) whose poses
it reads from `*-pose_icp.txt` files written by an external program. This is that stage as a device computation: a projective
point-to-plane ICP between the depth of the current pose, drawn by the rasteriser, and the sensor depth. It serves as
"DeepIM + ICP" on the network's final poses (TEST.DEPTH_ICP, core/tester.py) and as an "ICP only" baseline on initial poses.
"""
from __future__ import print_function, division, absolute_import

import ctypes

import numpy as np

from ...runtime import DeviceArray, lib


class DepthICP(object):
    """refine(poses, class_index, depth_observed) → (poses_refined, status), all on the device and without a read-back.

    Per call the normals of the observed depth are computed once (deepim_depth_normals). Each of the `outer` rounds draws the
    depth of the current poses (Render_Py.render_classes_into, device class ids), resets the increment T to the identity, runs
    `inner` Gauss-Newton steps of it against that one drawn depth (deepim_icp_step) and applies it (deepim_icp_apply).

    dist_max (m): a source point and the target vertex it projects onto are a pair only when closer than this — it is also what
    drops the background when the observed depth is unmasked. max_step (m): the target has no normal where its depth jumps by
    more than this between neighbouring pixels. min_pairs, rcond: a system with fewer pairs (status 1) or with a Cholesky pivot
    <= rcond · max diag (status 2) is not solved and leaves the pose as it was. The defaults are starting values: the project
    has not tuned them on real LINEMOD depth.

    Buffers are allocated on the first call for its (B, H, W) and reused while the shape stays."""

    def __init__(self, render_machine, config, dist_max=0.02, max_step=0.01, min_pairs=12, rcond=1e-9, outer=2, inner=5):
        if render_machine is None:
            raise ValueError("DepthICP: a render_machine is required (it draws the depth of the current poses)")
        if outer < 1 or inner < 1:
            raise ValueError("DepthICP: outer and inner must be at least 1")
        self.render_machine, self.config = render_machine, config
        self.ctx = render_machine.ctx
        self.dist_max, self.max_step = float(dist_max), float(max_step)
        self.min_pairs, self.rcond = int(min_pairs), float(rcond)
        self.outer, self.inner = int(outer), int(inner)
        self._buf = None
        self._identity = None

    def _buffers(self, B, H, W):
        if self._buf is None or self._buf["depth"].shape != (B, 1, H, W):
            ctx = self.ctx
            self._buf = {"image": ctx.empty((B, 3, H, W)), "depth": ctx.empty((B, 1, H, W)), "normals": ctx.empty((B, 3, H, W)),
                         "T": ctx.empty((B, 3, 4)), "pose": ctx.empty((B, 3, 4)), "status": ctx.empty((B,), dtype=np.int32)}
            self._identity = ctx.array(np.tile(np.eye(3, 4, dtype=np.float32), (B, 1, 1)))
        return self._buf

    def refine(self, poses, class_index, depth_observed, K=None, skip=None, out=None):
        """poses (B,3,4) device (or host: uploaded); class_index device int32 (B), the render machine's class ids;
        depth_observed device (B,1,H,W) float32 metres, 0 = no measurement (it may be the raw, unmasked sensor depth).
        K: None (the render machine's), a host (3,3), or a DeviceArray (B,3,3) of per-pair cameras, bound as the context's camera
        table as calc_EPE_batch does. skip: device int32 (B) or None; a row with skip != 0 keeps its pose.
        out: device (B,3,4) for the refined poses (may be `poses`), allocated when None.
        → (out, status): status device int32 (B) of the last step — 0 solved, 1 too few pairs, 2 rank-deficient. The status array
        belongs to this object and is overwritten by the next call."""
        rm, ctx = self.render_machine, self.ctx
        B = poses.shape[0]
        H, W = rm.height, rm.width
        if not isinstance(depth_observed, DeviceArray) or depth_observed.dtype != np.float32 or depth_observed.size != B * H * W:
            raise ValueError("DepthICP.refine: depth_observed must be a device float32 (%d,1,%d,%d) array" % (B, H, W))
        if not isinstance(poses, DeviceArray):
            poses = ctx.array(np.asarray(poses, np.float32).reshape(B, 3, 4))
        if isinstance(K, DeviceArray):
            if K.shape != (B, 3, 3):
                raise ValueError("DepthICP.refine: a device K must be (%d,3,3), got %s" % (B, K.shape))
            Kd, Kh = K, None
        else:
            Kd, Kh = None, np.ascontiguousarray(rm.K if K is None else K, dtype=np.float32).reshape(3, 3)
        buf = self._buffers(B, H, W)
        if out is None:
            out = ctx.empty((B, 3, 4))
        h = ctx.handle
        if Kd is not None:
            ctx.bind_cameras(Kd)
        lib.deepim_depth_normals(h, buf["normals"], depth_observed, Kh, ctypes.c_float(self.max_step), B, H, W)
        cur = poses
        for rnd in range(self.outer):
            rm.render_classes_into(buf["image"], buf["depth"], class_index, cur, K=Kd if Kd is not None else Kh)
            buf["T"].copyfrom(self._identity)
            for _ in range(self.inner):
                lib.deepim_icp_step(h, buf["T"], None, buf["status"], buf["depth"], depth_observed, buf["normals"], Kh, skip,
                                    ctypes.c_float(self.dist_max), self.min_pairs, ctypes.c_double(self.rcond), B, H, W)
            nxt = out if rnd == self.outer - 1 else buf["pose"]
            lib.deepim_icp_apply(h, nxt, buf["T"], cur, B)
            cur = nxt
        return out, buf["status"]

"""Training metrics (deepim/core/metric.py:13-137, mx.metric.EvalMetric / CompositeEvalMetric) with their sums on the device.

The reference copies flow_loss (twice), mask_prob and mask_gt to the host once per batch and sums there. Here `update` is one
deepim_train_metrics call (csrc/metric.hip) that adds into device doubles; `num_inst` stays a host integer; `get()` is the only
place that reads back — one copy of ten doubles for a composite. `preds` is a dict name → DeviceArray under the reference's
output names (deepIM_flownet.train_outputs()); `labels` is not read, as in the reference.

Every batch is counted, including one whose fp16 / x3 optimizer step was skipped for a gradient overflow: the forward pass and
its losses of that batch exist whether or not the parameters moved, and the reference has no such step to compare with.
"""
import ctypes

import numpy as np

from ..runtime import lib

# slot order of deepim_train_metrics
SLOTS = ("flow_loss", "rot_loss", "trans_loss", "point_matching_loss", "mask")
_NSLOT = len(SLOTS)
_ARGS = ("flow_loss", "rot_loss", "trans_loss", "point_matching_loss", "mask_prob", "mask_gt")


def get_flow_names_iter(cfg):
    """metric.py:13-48 → (pred names, label names), the order of the training graph's outputs and labels."""
    net, it = cfg.network, cfg.train_iter
    label = ["mask_real_gt"] if net.PRED_MASK else []
    label += ["rot", "trans"]
    if net.PRED_FLOW:
        label += ["flow", "flow_weight"]
    if it.SE3_PM_LOSS:
        label += ["point_cloud_model", "point_cloud_weights", "point_cloud_real"]
    pred = ["image_real", "image_rendered"]
    if net.PRED_FLOW:
        pred += ["flow_est_crop", "flow_loss"]
    pred += ["rot_est", "rot_gt", "trans_est", "trans_gt"]
    if it["SE3_DIST_LOSS"]:
        pred += ["rot_loss", "trans_loss"]
    if it["SE3_PM_LOSS"]:
        pred.append("point_matching_loss")
    if net["INPUT_MASK"] and net["PRED_MASK"]:
        pred += ["mask_prob", "mask_gt", "mask_pred"]
    pred.append("debug_term")
    return pred, label


def _metrics_call(buf, preds, names, totals, step):
    """One deepim_train_metrics call into `buf` (ten doubles: totals, then step) with the tensors `names` of preds."""
    args = []
    for key in _ARGS:
        a = preds[key] if key in names else None
        args.append(a)
        if key != "mask_prob":
            args.append(0 if a is None else a.size)
    lib.deepim_train_metrics(buf.context.handle, ctypes.c_void_p(buf.ptr) if totals else None,
                             ctypes.c_void_p(buf.ptr + 8 * _NSLOT) if step else None, *args)


class EvalMetric(object):
    """mx.metric.EvalMetric: name, reset, update, get, get_name_value. sum_metric is a device double (read it through
    `sum_metric`, which copies), num_inst a host integer; get() is NaN while num_inst == 0."""

    inputs = ()        # the preds this metric reads
    slot = 0           # its slot of deepim_train_metrics
    from_step = False  # True: the value is the last batch's sum, not the running total

    def __init__(self, name):
        self.name = str(name)
        self._buf = None
        self.num_inst = 0

    def _buffer(self, ctx):
        if self._buf is None:
            self._buf = ctx.zeros((2 * _NSLOT,), np.float64)
        return self._buf

    def _cell(self):
        return self.slot + (_NSLOT if self.from_step else 0)

    def reset(self):
        """num_inst = 0 and the metric's device double zeroed on the stream (no synchronisation)."""
        self.num_inst = 0
        if self._buf is not None:
            lib.deepim_memset(self._buf.context.handle, ctypes.c_void_p(self._buf.ptr + 8 * self._cell()), 0, 8)

    def _count(self):
        raise NotImplementedError

    def update(self, labels, preds):
        buf = self._buffer(preds[self.inputs[0]].context)
        _metrics_call(buf, preds, self.inputs, totals=not self.from_step, step=self.from_step)
        self._count()

    def _value(self, host):
        return float("nan") if self.num_inst == 0 else float(host[self._cell()]) / self.num_inst

    @property
    def sum_metric(self):
        return 0.0 if self._buf is None else float(self._buf.asnumpy()[self._cell()])

    def get(self):
        if self.num_inst == 0 or self._buf is None:
            return self.name, float("nan")
        return self.name, self._value(self._buf.asnumpy())

    def get_name_value(self):
        name, value = self.get()
        return [(name, value)]


class CompositeEvalMetric(EvalMetric):
    """mx.metric.CompositeEvalMetric over the metrics below: update is ONE deepim_train_metrics call for all children into one
    buffer of ten doubles (five running totals, five sums of the last batch), get() one copy of it."""

    def __init__(self, metrics=None, name="composite"):
        super(CompositeEvalMetric, self).__init__(name)
        self.metrics = []
        for m in metrics or []:
            self.add(m)

    def add(self, metric):
        self.metrics.append(metric)

    def get_metric(self, index):
        return self.metrics[index]

    def reset(self):
        for m in getattr(self, "metrics", []):
            m.num_inst = 0
        if self._buf is not None:
            lib.deepim_memset(self._buf.context.handle, self._buf, 0, self._buf.nbytes)

    def update(self, labels, preds):
        if not self.metrics:
            return
        names = {k for m in self.metrics for k in m.inputs}
        buf = self._buffer(preds[self.metrics[0].inputs[0]].context)
        for m in self.metrics:       # the children read (and, updated alone, add into) the composite's buffer
            m._buf = buf
        _metrics_call(buf, preds, names, totals=True, step=True)
        for m in self.metrics:
            m._count()

    def get(self):
        host = None if self._buf is None else self._buf.asnumpy()
        names = [m.name for m in self.metrics]
        if host is None:
            return names, [float("nan")] * len(names)
        return names, [m._value(host) for m in self.metrics]

    def get_name_value(self):
        names, values = self.get()
        return list(zip(names, values))


class _LossMetric(EvalMetric):
    """The reference's constructor (cfg, iter_idx=-1) and attributes."""

    metric_name = None

    def __init__(self, cfg, iter_idx=-1):
        super(_LossMetric, self).__init__(self.metric_name)
        self.pred, self.label = get_flow_names_iter(cfg)
        self.iter_idx = iter_idx
        self.show_interval = cfg.default.frequent


class Flow_L2LossMetric(_LossMetric):            # metric.py:51-63
    metric_name, inputs, slot = "Flow_L2Loss", ("flow_loss",), 0

    def _count(self):
        self.num_inst += 480 * 640


class Flow_CurLossMetric(_LossMetric):           # metric.py:66-77: the last batch only
    metric_name, inputs, slot, from_step = "Flow_CurLoss", ("flow_loss",), 0, True

    def _count(self):
        self.num_inst = 480 * 640


class Rot_L2LossMetric(_LossMetric):             # metric.py:80-91
    metric_name, inputs, slot = "Rot_L2Loss", ("rot_loss",), 1

    def _count(self):
        self.num_inst += 1


class Trans_L2LossMetric(_LossMetric):           # metric.py:94-105
    metric_name, inputs, slot = "Trans_L2Loss", ("trans_loss",), 2

    def _count(self):
        self.num_inst += 1


class PointMatchingLossMetric(_LossMetric):      # metric.py:108-120
    metric_name, inputs, slot = "PointMatchingLoss", ("point_matching_loss",), 3

    def __init__(self, cfg, iter_idx=-1):
        super(PointMatchingLossMetric, self).__init__(cfg, iter_idx)
        self.sample_per_iter = cfg["train_iter"]["NUM_3D_SAMPLE"]

    def _count(self):
        self.num_inst += self.sample_per_iter


class MaskLossMetric(_LossMetric):               # metric.py:123-137
    metric_name, inputs, slot = "MaskLoss", ("mask_prob", "mask_gt"), 4

    def _count(self):
        self.num_inst += 480 * 640

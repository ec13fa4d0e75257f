#!/usr/bin/env python
"""Golden vectors of the training loop's metrics, Speedometer and learning-rate schedule, produced by running the REFERENCE'S OWN
deepim/core/metric.py, deepim/core/callback.py and lib/utils/lr_scheduler.py.

Runs only in the build container (needs /root/reference):  python tests/golden/make_train_metrics_golden.py
Writes tests/golden/train_metrics_golden.npz (committed; data only).  TEST INFRASTRUCTURE ONLY.

The three files are imported UNMODIFIED. What they import and is not installed is a stand-in put into sys.modules first
(make_flow_epe_golden.py is the precedent): `mxnet` with a minimal metric.EvalMetric (name, reset → num_inst = 0 and
sum_metric = 0.0, get) and lr_scheduler.LRScheduler (base_lr), `lib.utils.logger` whose info() keeps the formatted line, and a
stepped time.time inside callback.py.

Metrics. Per metric three consecutive update() calls on small float32 tensors (stored as u<k>_<name>), with sum_metric and
num_inst after each (ref_<Metric>_sum / _num). Next to each reference sum the file holds the float64 sum of the SAME float32
elements (f64_<Metric>_sum; for MaskLoss the elements are metric.py:135 evaluated by numpy in float32). main() asserts that the
two agree within 2e-7 relative: the reference's own float32 summation error on these inputs. That is a condition on the
inputs, not a bar for the kernel. The mask inputs contain p exactly 0, exactly 1, 1 - 2^-24 and 1e-30, and g of 0, 1 and
fractions.

Speedometer: the lines of a run over two epochs with frequent = 2 (and one without a metric), under a clock that advances by
a stored step per call. Scheduler: the lr for sequences of num_update with warm-up, a boundary crossed inside a batch of four
updates, and a jump past two boundaries, with the lines it logs.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mx_deepim_amd.config import AttrDict  # noqa: E402

LINES = []     # what the stand-in logger was told


def install_stand_ins():
    class EvalMetric(object):
        def __init__(self, name, num=None):
            self.name = name
            self.num = num
            self.reset()

        def reset(self):
            self.num_inst = 0
            self.sum_metric = 0.0

        def get(self):
            if self.num_inst == 0:
                return (self.name, float("nan"))
            return (self.name, self.sum_metric / self.num_inst)

    class LRScheduler(object):
        def __init__(self, base_lr=0.01):
            self.base_lr = base_lr

    mx = types.ModuleType("mxnet")
    mx.metric = types.ModuleType("mxnet.metric")
    mx.metric.EvalMetric = EvalMetric
    mx.lr_scheduler = types.ModuleType("mxnet.lr_scheduler")
    mx.lr_scheduler.LRScheduler = LRScheduler
    sys.modules.update({"mxnet": mx, "mxnet.metric": mx.metric, "mxnet.lr_scheduler": mx.lr_scheduler})

    lib = types.ModuleType("lib")
    lib.utils = types.ModuleType("lib.utils")
    log = types.ModuleType("lib.utils.logger")
    log.info = lambda fmt, *args: LINES.append(fmt % args if args else fmt)
    lib.utils.logger = log
    sys.modules.update({"lib": lib, "lib.utils": lib.utils, "lib.utils.logger": log})


def load_reference(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Arr(object):
    def __init__(self, a):
        self.a = a

    def asnumpy(self):
        return self.a


def make_cfg():
    cfg = AttrDict()
    cfg.default = AttrDict(frequent=20)
    cfg.network = AttrDict(PRED_MASK=True, PRED_FLOW=True, INPUT_MASK=True)
    cfg.train_iter = AttrDict(SE3_PM_LOSS=True, SE3_DIST_LOSS=True, NUM_3D_SAMPLE=3000)
    return cfg


def make_tensors(rng, k):
    """The float32 outputs of update k: sizes that differ per tensor and per update."""
    B = 2 + k
    f32 = np.float32
    t = {"flow_loss": (rng.random((B, 2, 13, 17 + k)) ** 3 * 5.0).astype(f32),
         "rot_loss": (rng.random((B,)) * 0.3).astype(f32),
         "trans_loss": (rng.random((B, 3, 1)) * 0.02).astype(f32),
         "point_matching_loss": (rng.random((B, 3, 91 + 100 * k)) * 0.004).astype(f32)}
    n = B * 11 * (19 + k)
    p = rng.random(n).astype(f32)
    g = (rng.random(n) > 0.6).astype(f32)
    frac = rng.random(n) < 0.15                     # zoomed ground truth: fractions at the edges
    g[frac] = rng.random(int(frac.sum())).astype(f32)
    special_p = np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 1e-30, 0.0, 1.0, 1.0 - 2.0 ** -24, 1e-30, 0.0, 1.0, 0.5], f32)
    special_g = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.25, 0.75, 0.5], f32)
    at = rng.choice(n, special_p.size, replace=False)
    p[at], g[at] = special_p, special_g
    t["mask_prob"], t["mask_gt"] = p.reshape(B, 1, 11, 19 + k), g.reshape(B, 1, 11, 19 + k)
    return t


def mask_elements(p, g):
    return -(g * np.log(p + 1e-19) + (1 - g) * np.log(1 - p + 1e-19))


def run_metrics(metric, out):
    cfg = make_cfg()
    classes = [("Flow_L2Loss", metric.Flow_L2LossMetric, "flow_loss"), ("Flow_CurLoss", metric.Flow_CurLossMetric, "flow_loss"),
               ("Rot_L2Loss", metric.Rot_L2LossMetric, "rot_loss"), ("Trans_L2Loss", metric.Trans_L2LossMetric, "trans_loss"),
               ("PointMatchingLoss", metric.PointMatchingLossMetric, "point_matching_loss"),
               ("MaskLoss", metric.MaskLossMetric, "mask")]
    pred_names, label_names = metric.get_flow_names_iter(cfg)
    out["pred_names"], out["label_names"] = np.array(pred_names), np.array(label_names)
    rng = np.random.default_rng(2121)
    tensors = [make_tensors(rng, k) for k in range(3)]
    for k, t in enumerate(tensors):
        for name, a in t.items():
            out["u%d_%s" % (k, name)] = a
    for mname, cls, src in classes:
        m = cls(cfg, 0)
        assert m.name == mname
        name0, value0 = m.get()
        assert np.isnan(value0)
        sums, nums, f64s, run = [], [], [], 0.0
        for t in tensors:
            preds = [Arr(t.get(n)) for n in pred_names]
            m.update(None, preds)
            sums.append(float(m.sum_metric))
            nums.append(int(m.num_inst))
            elems = mask_elements(t["mask_prob"], t["mask_gt"]) if src == "mask" else t[src]
            assert elems.dtype == np.float32 and np.all(np.isfinite(elems))
            s = float(np.sum(elems.astype(np.float64)))
            run = s if mname == "Flow_CurLoss" else run + s
            f64s.append(run)
        gap = np.abs(np.array(sums) - np.array(f64s)) / np.abs(np.array(f64s))
        assert gap.max() <= 2e-7, (mname, gap)
        print("%-18s reference sums against float64 sums of the same elements: %.2e" % (mname, gap.max()))
        out["ref_%s_sum" % mname], out["ref_%s_num" % mname] = np.array(sums, np.float64), np.array(nums, np.int64)
        out["f64_%s_sum" % mname] = np.array(f64s, np.float64)
        out["ref_%s_get" % mname] = np.float64(m.get()[1])
    out["num_3d_sample"] = np.int64(cfg.train_iter.NUM_3D_SAMPLE)


class StubMetric(object):
    def __init__(self, names, values):
        self.names, self.values = names, values

    def get(self):
        return self.names, self.values


def run_speedometer(callback, out):
    steps = [0.5, 0.25, 1.0, 2.0, 0.125, 4.0, 0.75]
    state = {"now": 1000.0, "i": 0}

    def stepped():
        state["now"] += steps[state["i"] % len(steps)]
        state["i"] += 1
        return state["now"]

    callback.time = types.SimpleNamespace(time=stepped)
    names = ["Flow_L2Loss", "Flow_CurLoss", "PointMatchingLoss", "MaskLoss"]
    Param = lambda epoch, nbatch, m: types.SimpleNamespace(epoch=epoch, nbatch=nbatch, eval_metric=m)   # noqa: E731
    calls, values = [], []
    sp = callback.Speedometer(4, frequent=2)
    del LINES[:]
    i = 0
    for epoch in range(2):
        for nbatch in range(5):
            v = [0.0123456789 * (i + 1), 1.5 / (i + 1), float("nan") if i == 2 else 3e-7 * (i + 1), 12345.678 + i]
            calls.append((epoch, nbatch, 1))
            values.append(v)
            sp(Param(epoch, nbatch, StubMetric(names, v)))
            i += 1
    for nbatch in range(3):          # without a metric: the "Iter" line
        calls.append((2, nbatch, 0))
        values.append([0.0] * 4)
        sp(Param(2, nbatch, None))
    out["speed_steps"], out["speed_t0"] = np.array(steps, np.float64), np.float64(1000.0)
    out["speed_batch_size"], out["speed_frequent"] = np.int64(4), np.int64(2)
    out["speed_names"] = np.array(names)
    out["speed_calls"], out["speed_values"] = np.array(calls, np.int64), np.array(values, np.float64)
    out["speed_lines"] = np.array(list(LINES))
    assert len(LINES) == 5, LINES


def run_scheduler(sched_mod, out):
    cases = {
        # warm-up, then two boundaries walked one update at a time
        "warm": dict(step=[6, 10], factor=0.1, warmup=True, warmup_lr=1e-5, warmup_step=3, base_lr=1e-3, seq=list(range(0, 14))),
        # batches of four updates: the batch-start query with the count so far, then its four updates; 6 lies inside batch 1
        "batch4": dict(step=[6], factor=0.5, warmup=False, warmup_lr=0.0, warmup_step=0, base_lr=2e-4,
                       seq=[0, 1, 2, 3, 4, 4, 5, 6, 7, 8, 8, 9, 10, 11, 12]),
        # one call jumps past two boundaries (the while loop)
        "jump": dict(step=[3, 5, 20], factor=0.1, warmup=False, warmup_lr=0.0, warmup_step=0, base_lr=0.01, seq=[1, 9, 10, 25, 26]),
    }
    out["sched_cases"] = np.array(sorted(cases))
    for tag, c in cases.items():
        s = sched_mod.WarmupMultiFactorScheduler(list(c["step"]), c["factor"], c["warmup"], c["warmup_lr"], c["warmup_step"])
        s.base_lr = c["base_lr"]          # mx.optimizer.Optimizer.__init__ hands its learning_rate over
        del LINES[:]
        lrs = [float(s(n)) for n in c["seq"]]
        out["sched_%s_step" % tag] = np.array(c["step"], np.int64)
        out["sched_%s_args" % tag] = np.array([c["factor"], float(c["warmup"]), c["warmup_lr"], c["warmup_step"], c["base_lr"]],
                                              np.float64)
        out["sched_%s_seq" % tag] = np.array(c["seq"], np.int64)
        out["sched_%s_lr" % tag] = np.array(lrs, np.float64)
        out["sched_%s_lines" % tag] = np.array(list(LINES) or [""])
        out["sched_%s_nlines" % tag] = np.int64(len(LINES))


def main():
    install_stand_ins()
    metric = load_reference("ref_metric", "deepim/core/metric.py")
    callback = load_reference("ref_callback", "deepim/core/callback.py")
    sched = load_reference("ref_lr_scheduler", "lib/utils/lr_scheduler.py")
    out = {}
    run_metrics(metric, out)
    run_speedometer(callback, out)
    run_scheduler(sched, out)
    path = os.path.join(HERE, "train_metrics_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()

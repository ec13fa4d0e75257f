"""numpy restatement of deepim_train_metrics and deepim_l2_norms_multi (csrc/metric.hip) and of the metric classes above them
(mx_deepim_amd/core/metric.py): elements as numpy computes them on float32 inputs, sums in float64. Shared by
tests/test_train_metrics_host.py (against the reference-run fixture, on the CPU) and tests/test_gpu_train_metrics.py /
tests/test_gpu_fit.py (the GPU against this)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_metrics_golden.npz")
SLOTS = ("flow_loss", "rot_loss", "trans_loss", "point_matching_loss", "mask")
# metric name → (slot, running total (False: the last batch only), num_inst per update; None = train_iter.NUM_3D_SAMPLE)
METRICS = {"Flow_L2Loss": (0, True, 480 * 640), "Flow_CurLoss": (0, False, 480 * 640), "Rot_L2Loss": (1, True, 1),
           "Trans_L2Loss": (2, True, 1), "PointMatchingLoss": (3, True, None), "MaskLoss": (4, True, 480 * 640)}


def mask_elements(p, g):
    """deepim/core/metric.py:135 on float32 arrays: every operation float32 (1e-19 is a Python float, so numpy keeps float32)."""
    p, g = np.asarray(p), np.asarray(g)
    assert p.dtype == np.float32 and g.dtype == np.float32
    out = -(g * np.log(p + 1e-19) + (1 - g) * np.log(1 - p + 1e-19))
    assert out.dtype == np.float32
    return out


def sum64(x):
    return float(np.sum(np.asarray(x, np.float32).astype(np.float64)))


def train_metrics(flow_loss=None, rot_loss=None, trans_loss=None, pm_loss=None, mask_prob=None, mask_gt=None):
    """→ the five float64 sums of one call (`step`; 0 for an absent tensor)."""
    out = [0.0 if a is None else sum64(a) for a in (flow_loss, rot_loss, trans_loss, pm_loss)]
    out.append(0.0 if mask_prob is None else sum64(mask_elements(mask_prob, mask_gt)))
    return np.array(out, np.float64)


def step_of_preds(preds):
    """The same from a dict under the reference's output names (deepIM_flownet.train_outputs() read back)."""
    return train_metrics(preds.get("flow_loss"), preds.get("rot_loss"), preds.get("trans_loss"),
                         preds.get("point_matching_loss"), preds.get("mask_prob"), preds.get("mask_gt"))


def metric_history(name, steps, num_3d_sample=3000):
    """(sum_metric, num_inst) of metric `name` after each of the updates whose sums are the rows of `steps`."""
    slot, running, per = METRICS[name]
    per = num_3d_sample if per is None else per
    sums, nums, s, n = [], [], 0.0, 0
    for row in steps:
        s = s + row[slot] if running else row[slot]
        n = n + per if running else per
        sums.append(s)
        nums.append(n)
    return np.array(sums, np.float64), np.array(nums, np.int64)


def l2_norm(x):
    """float32(sqrt) of the float64 sum of squares rounded to float32, as deepim_l2_norms_multi."""
    x = np.asarray(x, np.float32).astype(np.float64)
    return np.sqrt(np.float32(np.sum(x * x)))


def fixture_steps(gold):
    """The three updates of the fixture → (3, 5) float64 sums."""
    return np.stack([train_metrics(gold["u%d_flow_loss" % k], gold["u%d_rot_loss" % k], gold["u%d_trans_loss" % k],
                                   gold["u%d_point_matching_loss" % k], gold["u%d_mask_prob" % k], gold["u%d_mask_gt" % k])
                     for k in range(3)])


def fixture_preds(gold, k):
    return {n: gold["u%d_%s" % (k, n)] for n in ("flow_loss", "rot_loss", "trans_loss", "point_matching_loss", "mask_prob",
                                                 "mask_gt")}


def stepped_clock(gold):
    """The generator's clock: advances by the next stored step per call."""
    steps, state = gold["speed_steps"], {"now": float(gold["speed_t0"]), "i": 0}

    def now():
        state["now"] += float(steps[state["i"] % len(steps)])
        state["i"] += 1
        return state["now"]

    return now

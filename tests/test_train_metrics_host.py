"""Training metrics, Speedometer and the learning-rate schedule without a GPU, against what the reference's own metric.py,
callback.py and lr_scheduler.py gave (tests/golden/train_metrics_golden.npz, made by tests/golden/make_train_metrics_golden.py).

The numpy restatement of the device reduction (tests/train_metrics_emulation.py: elements in float32 as numpy evaluates them,
sums in float64) reproduces every reference sum within 2e-7 relative: the reference adds in float32, and the generator asserts
that bound against the float64 sum of the same elements. The scheduler and Speedometer are pure host code and must equal the
fixture exactly: every lr, every line."""
import logging
import types

import numpy as np
import pytest

import train_metrics_emulation as emu
from mx_deepim_amd.config import default_config
from mx_deepim_amd.core import callback as cb
from mx_deepim_amd.core import metric
from mx_deepim_amd.lib.utils.lr_scheduler import WarmupMultiFactorScheduler, lr_schedule


@pytest.fixture(scope="module")
def gold():
    return np.load(emu.GOLDEN)


class _Lines(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _logger(name):
    lg, h = logging.getLogger(name), _Lines()
    lg.handlers, lg.propagate = [h], False
    lg.setLevel(logging.INFO)
    return lg, h.lines


@pytest.mark.parametrize("name", sorted(emu.METRICS))
def test_restatement_reproduces_the_reference_metric(gold, name):
    sums, nums = emu.metric_history(name, emu.fixture_steps(gold), int(gold["num_3d_sample"]))
    ref = gold["ref_%s_sum" % name]
    np.testing.assert_array_equal(nums, gold["ref_%s_num" % name])
    assert np.all(np.abs(sums - ref) <= 2e-7 * np.abs(ref)), (sums, ref)
    # the float64 sums the generator stored next to the reference's are the restatement's, to a few ulp of double
    np.testing.assert_allclose(sums, gold["f64_%s_sum" % name], rtol=1e-13)
    assert abs(sums[-1] / nums[-1] - float(gold["ref_%s_get" % name])) <= 2e-7 * abs(float(gold["ref_%s_get" % name]))


def test_mask_elements_at_the_special_probabilities():
    p = np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 1e-30], np.float32)
    for g in (0.0, 1.0, 0.25):
        e = emu.mask_elements(p, np.full(4, g, np.float32))
        assert np.all(np.isfinite(e)) and np.all(e >= 0)
    big = np.float32(-np.log(np.float32(1e-19)))
    assert emu.mask_elements(p[1:2], np.zeros(1, np.float32))[0] == big      # p == 1, g == 0: log(1e-19f), not log(0)
    assert emu.mask_elements(p[0:1], np.ones(1, np.float32))[0] == big


def test_names_of_outputs_and_labels(gold):
    cfg = default_config()
    cfg.train_iter.SE3_DIST_LOSS = True
    pred, label = metric.get_flow_names_iter(cfg)
    assert pred == list(gold["pred_names"]) and label == list(gold["label_names"])
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = False
    cfg.train_iter.SE3_DIST_LOSS = False
    pred, label = metric.get_flow_names_iter(cfg)
    assert pred == ["image_real", "image_rendered", "rot_est", "rot_gt", "trans_est", "trans_gt", "point_matching_loss",
                    "debug_term"]
    assert label == ["rot", "trans", "point_cloud_model", "point_cloud_weights", "point_cloud_real"]


def test_metric_classes_before_any_update():
    cfg = default_config()
    comp = metric.CompositeEvalMetric()
    for cls in (metric.Flow_L2LossMetric, metric.Flow_CurLossMetric, metric.Rot_L2LossMetric, metric.Trans_L2LossMetric,
                metric.PointMatchingLossMetric, metric.MaskLossMetric):
        m = cls(cfg, 0)
        assert m.iter_idx == 0 and m.show_interval == cfg.default.frequent and m.num_inst == 0
        name, value = m.get()
        assert name == cls.metric_name and np.isnan(value)
        comp.add(m)
    names, values = comp.get()
    assert names == sorted(emu.METRICS, key=lambda n: (emu.METRICS[n][0], not emu.METRICS[n][1]))
    assert len(values) == 6 and all(np.isnan(v) for v in values)
    comp.reset()
    assert comp.get_name_value()[0][0] == "Flow_L2Loss"


@pytest.mark.parametrize("tag", ["warm", "batch4", "jump"])
def test_scheduler_equals_the_reference(gold, tag):
    factor, warmup, warmup_lr, warmup_step, base_lr = gold["sched_%s_args" % tag]
    lg, lines = _logger("test_sched_" + tag)
    s = WarmupMultiFactorScheduler([int(x) for x in gold["sched_%s_step" % tag]], factor, bool(warmup), warmup_lr, warmup_step,
                                   logger=lg)
    s.base_lr = base_lr
    lrs = np.array([s(int(n)) for n in gold["sched_%s_seq" % tag]], np.float64)
    np.testing.assert_array_equal(lrs, gold["sched_%s_lr" % tag])
    assert lines == list(gold["sched_%s_lines" % tag])[:int(gold["sched_%s_nlines" % tag])]


def test_scheduler_checks():
    with pytest.raises(AssertionError):
        WarmupMultiFactorScheduler([])
    with pytest.raises(ValueError, match="increasing"):
        WarmupMultiFactorScheduler([4, 4])
    with pytest.raises(ValueError, match="greater or equal than 1"):
        WarmupMultiFactorScheduler([0, 3])
    with pytest.raises(ValueError, match="no more than 1"):
        WarmupMultiFactorScheduler([3], factor=1.5)
    assert WarmupMultiFactorScheduler([3]).base_lr == 0.01


def test_speedometer_equals_the_reference(gold, monkeypatch):
    monkeypatch.setattr(cb, "time", types.SimpleNamespace(time=emu.stepped_clock(gold)))
    lg, lines = _logger("test_speedometer")
    sp = cb.Speedometer(int(gold["speed_batch_size"]), frequent=int(gold["speed_frequent"]), logger=lg)
    names = list(gold["speed_names"])
    for (epoch, nbatch, has), values in zip(gold["speed_calls"], gold["speed_values"]):
        m = types.SimpleNamespace(get=lambda v=values: (names, list(v))) if has else None
        sp(types.SimpleNamespace(epoch=int(epoch), nbatch=int(nbatch), eval_metric=m))
    assert lines == list(gold["speed_lines"])


def test_lr_schedule_arithmetic_of_train_py():
    # fresh run: 8 epochs, boundaries at 4 and 6, 1000 pairs on one device
    lr, lr_epoch, diff, iters = lr_schedule(1e-4, "4, 6", 0, 1000)
    assert (lr, lr_epoch, diff, iters) == (1e-4, [4.0, 6.0], [4.0, 6.0], [4000, 6000])
    # resumed at epoch 5: one boundary passed (lr · 0.1), the other one epoch ahead; updates count from 0 again
    lr, lr_epoch, diff, iters = lr_schedule(1e-4, "4, 6", 5, 1000)
    assert lr == 1e-4 * (0.1 ** 1) and diff == [1.0] and iters == [1000]
    # resumed exactly at a boundary: `epoch > begin_epoch` drops it
    lr, _, diff, iters = lr_schedule(1e-4, "4, 6", 4, 1000)
    assert lr == 1e-4 * 0.1 and diff == [2.0] and iters == [2000]
    # several devices and a fractional epoch: int() truncates
    lr, _, diff, iters = lr_schedule(2e-3, "1.5,3", 0, 1001, num_gpus=4)
    assert lr == 2e-3 and diff == [1.5, 3.0] and iters == [int(1.5 * 1001 / 4), int(3.0 * 1001 / 4)] == [375, 750]
    # past every boundary: nothing left (WarmupMultiFactorScheduler then refuses the empty list, as the reference's does)
    lr, _, diff, iters = lr_schedule(1e-4, "4, 6", 7, 1000)
    assert lr == 1e-4 * (0.1 ** 2) and diff == [] and iters == []


def test_module_checkpoint_numbers_its_files_from_epoch_plus_one():
    calls = []
    mod = types.SimpleNamespace(save_checkpoint=lambda prefix, epoch, states: calls.append((prefix, epoch, states)))
    f = cb.module_checkpoint(mod, "out/net", period=2, save_optimizer_states=True)
    for epoch in (-1, 0, 1, 2, 3):
        f(epoch, None, None, None)
    assert calls == [("out/net", 0, True), ("out/net", 2, True), ("out/net", 4, True)]     # (epoch + 1) % period == 0
    calls[:] = []
    f = cb.module_checkpoint(mod, "p")
    f(-1)
    f(0)
    assert calls == [("p", 0, True), ("p", 1, True)]

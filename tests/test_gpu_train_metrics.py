"""deepim_train_metrics and deepim_l2_norms_multi on the GPU against their numpy restatement (tests/train_metrics_emulation.py),
and the metric classes (mx_deepim_amd/core/metric.py) against what the reference's own metric.py gave
(tests/golden/train_metrics_golden.npz).

Bars. Slots 0-3 add the same float32 elements in double in another order: n·2^-53 of Σ|x|, bar 1e-10. Slot 4: every term is
>= 0 and the device's logf is within a few ulp of numpy's float32 log, bar 5e-7 relative. Against the fixture the reference's
own float32 summation error (2e-7, asserted by the generator) is added. The norms: one float32 rounding of a double sum and one
sqrtf against float64 numpy, bar 1.2e-7 relative."""
import ctypes

import numpy as np
import pytest

import train_metrics_emulation as emu
from mx_deepim_amd.config import default_config
from mx_deepim_amd.core import metric
from mx_deepim_amd.runtime import DeviceArray, lib

pytestmark = pytest.mark.gpu

# lengths of the five slots: under a quad, a wave straddle, one past a block of quads, a lane walking several quads with a scalar
# tail, several blocks; mixed so that the slots of a call differ
CASES = [(100233, 1, 3, 91, 2145), (0, 3, 1025, 2145, 100233), (1025, 91, 0, 1, 3), (2145, 1025, 100233, 0, 91),
         (3, 2145, 91, 100233, 1025), (91, 0, 1, 3, 0), (1, 100233, 2145, 1025, 1)]
SPECIAL_P = np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 1e-30], np.float32)


def odd_slice(ctx, host, offset):
    """`host` (1-D float32) on the device at `offset` floats into a larger buffer: 4-byte aligned, not 16."""
    big = ctx.array(np.concatenate([np.full(offset, 7.5, np.float32), host, np.full(5, -3.25, np.float32)]))
    return DeviceArray(ctx, host.shape, np.float32, ptr=big.ptr + 4 * offset, base=big)


def host_tensors(lengths, seed):
    rng = np.random.default_rng(seed)
    t = [((rng.random(n) - 0.3) * 4.0).astype(np.float32) for n in lengths[:4]]
    n = lengths[4]
    p = rng.random(n).astype(np.float32)
    g = np.where(rng.random(n) < 0.2, rng.random(n), rng.random(n) > 0.5).astype(np.float32)
    k = min(n, 4)
    p[:k] = SPECIAL_P[:k]
    if n >= 8:
        p[-4:], g[-4:] = SPECIAL_P, np.array([1.0, 0.0, 1.0, 1.0], np.float32)
    return t + [p, g]


@pytest.fixture(scope="module")
def cases(ctx):
    """Per case the host tensors, their device slices and the restatement's five sums: computed once, never written."""
    out = []
    for i, lengths in enumerate(CASES):
        host = host_tensors(lengths, 400 + i)
        dev = [odd_slice(ctx, a, 1 + 2 * ((i + j) % 2)) for j, a in enumerate(host)]
        out.append((host, dev, emu.train_metrics(*host)))
    return out


def call(ctx, totals, step, dev, present=(1, 1, 1, 1, 1)):
    args = []
    for s in range(4):
        args += [dev[s] if present[s] else None, dev[s].size if present[s] else 0]
    args += [dev[4] if present[4] else None, dev[5] if present[4] else None, dev[4].size if present[4] else 0]
    lib.deepim_train_metrics(ctx.handle, totals, step, *args)


def check_step(got, host, want):
    for s in range(4):
        bar = 1e-10 * float(np.sum(np.abs(host[s].astype(np.float64))))
        print("slot %d n %6d: |got - want| %.3e, bar %.3e" % (s, host[s].size, abs(got[s] - want[s]), bar))
        assert abs(got[s] - want[s]) <= bar, s
    print("slot 4 n %6d: relative %.3e, bar 5e-7" % (host[4].size, abs(got[4] - want[4]) / max(abs(want[4]), 1e-300)))
    assert abs(got[4] - want[4]) <= 5e-7 * abs(want[4])


@pytest.mark.parametrize("i", range(len(CASES)))
def test_sums_against_the_restatement(ctx, cases, i):
    host, dev, want = cases[i]
    totals, step = ctx.zeros((5,), np.float64), ctx.empty((5,), np.float64)
    call(ctx, totals, step, dev)
    got = step.asnumpy()
    assert np.all(np.isfinite(got))
    check_step(got, host, want)
    np.testing.assert_array_equal(totals.asnumpy(), got)      # 0 + step
    for s, n in enumerate(CASES[i]):
        if n == 0:
            assert got[s] == 0.0


def test_mask_term_at_the_special_probabilities(ctx):
    """One element per call: p of 0, 1, 1 - 2^-24 and 1e-30 against g of 0, 1 and a fraction: finite, and numpy's value to 8 ulp."""
    step = ctx.empty((5,), np.float64)
    for p in SPECIAL_P:
        for g in (0.0, 1.0, 0.25):
            hp, hg = np.array([p], np.float32), np.array([g], np.float32)
            lib.deepim_train_metrics(ctx.handle, None, step, None, 0, None, 0, None, 0, None, 0, ctx.array(hp), ctx.array(hg), 1)
            got, want = step.asnumpy()[4], float(emu.mask_elements(hp, hg)[0])
            assert np.isfinite(got) and abs(got - want) <= 8 * 2.0 ** -24 * abs(want), (p, g, got, want)


def test_null_slots_leave_totals_alone_and_zero_step(ctx, cases):
    host, dev, want = cases[0]
    start = np.array([1.5, -2.25, 3.0, 4.125, 5.0])
    for present in [(1, 0, 1, 0, 0), (0, 1, 0, 0, 1), (0, 0, 0, 0, 0)]:
        totals, step = ctx.array(start, np.float64), ctx.array(np.full(5, 9.0), np.float64)
        call(ctx, totals, step, dev, present)
        t, s = totals.asnumpy(), step.asnumpy()
        full = ctx.empty((5,), np.float64)
        call(ctx, None, full, dev)
        full = full.asnumpy()
        for k in range(5):
            if present[k]:
                assert s[k] == full[k] and t[k] == start[k] + full[k]
            else:
                assert s[k] == 0.0 and t[k] == start[k]
    # totals alone, step alone, neither
    totals = ctx.array(start, np.float64)
    call(ctx, totals, None, dev)
    np.testing.assert_array_equal(totals.asnumpy(), start + full)
    call(ctx, None, None, dev)
    np.testing.assert_array_equal(totals.asnumpy(), start + full)


def test_two_calls_give_the_same_bytes_and_totals_add_in_order(ctx, cases):
    _h, dev_a, _w = cases[3]
    _h, dev_b, _w = cases[4]
    totals, step = ctx.zeros((5,), np.float64), ctx.empty((5,), np.float64)
    rows = []
    for dev in (dev_a, dev_b):
        call(ctx, totals, step, dev)
        rows.append(step.asnumpy())
    again = ctx.empty((5,), np.float64)
    call(ctx, None, again, dev_a)
    assert again.asnumpy().tobytes() == rows[0].tobytes()
    t = np.zeros(5)
    for row in rows:
        t = t + row
    np.testing.assert_array_equal(totals.asnumpy(), t)


def test_captured_graph_follows_a_rewritten_input(ctx, cases):
    host, _dev, _want = cases[2]
    dev = [ctx.array(a) for a in host]
    totals, step = ctx.zeros((5,), np.float64), ctx.empty((5,), np.float64)
    call(ctx, totals, step, dev)                   # eagerly once: the scratch grows outside the capture
    first = step.asnumpy()
    gid = ctypes.c_int(-1)
    lib.deepim_graph_begin(ctx.handle)
    try:
        call(ctx, totals, step, dev)
    finally:
        lib.deepim_graph_end(ctx.handle, ctypes.byref(gid))
    lib.deepim_graph_launch(ctx.handle, gid.value)
    np.testing.assert_array_equal(step.asnumpy(), first)
    host2 = [a.copy() for a in host]
    host2[0] = (host[0] * np.float32(0.5) + np.float32(0.25)).astype(np.float32)
    host2[4] = (host[4] * np.float32(0.5)).astype(np.float32)
    dev[0].copyfrom(host2[0])
    dev[4].copyfrom(host2[4])
    lib.deepim_graph_launch(ctx.handle, gid.value)
    second = step.asnumpy()
    assert second[0] != first[0] and second[4] != first[4] and second[1] == first[1]
    check_step(second, host2, emu.train_metrics(*host2))
    t = np.zeros(5)
    for row in (first, first, second):             # the eager call and two replays
        t = t + row
    np.testing.assert_array_equal(totals.asnumpy(), t)


# ---- the metric classes against the reference run
@pytest.fixture(scope="module")
def gold():
    return np.load(emu.GOLDEN)


@pytest.fixture(scope="module")
def gold_preds(ctx, gold):
    return [{k: ctx.array(v) for k, v in emu.fixture_preds(gold, u).items()} for u in range(3)]


def _cfg():
    cfg = default_config()
    cfg.train_iter.SE3_DIST_LOSS = True
    return cfg


CLASSES = [metric.Flow_L2LossMetric, metric.Flow_CurLossMetric, metric.Rot_L2LossMetric, metric.Trans_L2LossMetric,
           metric.PointMatchingLossMetric, metric.MaskLossMetric]


def _bar(name):
    return 2e-7 + (5e-7 if name == "MaskLoss" else 1e-10)


@pytest.mark.parametrize("cls", CLASSES, ids=[c.metric_name for c in CLASSES])
def test_metric_class_against_the_reference_run(ctx, gold, gold_preds, cls):
    m = cls(_cfg(), 0)
    assert np.isnan(m.get()[1])
    for u in range(3):
        m.update(None, gold_preds[u])
        ref = float(gold["ref_%s_sum" % m.name][u])
        print("%s update %d: sum %.17g reference %.17g relative %.3e" % (m.name, u, m.sum_metric, ref, abs(m.sum_metric - ref) / abs(ref)))
        assert m.num_inst == int(gold["ref_%s_num" % m.name][u])
        assert abs(m.sum_metric - ref) <= _bar(m.name) * abs(ref)
    ref_get = float(gold["ref_%s_get" % m.name])
    assert m.get()[0] == m.name and abs(m.get()[1] - ref_get) <= _bar(m.name) * abs(ref_get)
    m.reset()
    assert m.num_inst == 0 and np.isnan(m.get()[1]) and m.sum_metric == 0.0


def test_composite_equals_its_children_and_reads_back_once(ctx, gold, gold_preds, monkeypatch):
    cfg = _cfg()
    comp = metric.CompositeEvalMetric()
    for cls in CLASSES:
        comp.add(cls(cfg, 0))
    alone = [cls(cfg, 0) for cls in CLASSES]
    assert all(np.isnan(v) for v in comp.get()[1])
    comp.reset()
    reads = []
    real = DeviceArray.asnumpy
    monkeypatch.setattr(DeviceArray, "asnumpy", lambda self: (reads.append(self.nbytes), real(self))[1])
    for u in range(3):
        comp.update(None, gold_preds[u])
        for m in alone:
            m.update(None, gold_preds[u])
        assert reads == []                       # update never reads back
        names, values = comp.get()
        assert reads == [80]                     # one copy of the ten doubles
        del reads[:]
        assert names == [c.metric_name for c in CLASSES]
        for m, v in zip(alone, values):
            assert m.get()[1] == v, m.name           # the same partials in the same order: the same bits
        del reads[:]
    # Flow_CurLoss holds the last batch only
    last = emu.step_of_preds(emu.fixture_preds(gold, 2))
    cur = dict(comp.get_name_value())["Flow_CurLoss"]
    assert abs(cur * 480 * 640 - last[0]) <= 1e-10 * abs(last[0])
    comp.reset()
    assert all(np.isnan(v) for v in comp.get()[1])
    comp.update(None, gold_preds[0])
    first = metric.CompositeEvalMetric([cls(cfg, 0) for cls in CLASSES])
    first.update(None, gold_preds[0])
    assert comp.get()[1] == first.get()[1]           # reset zeroed the totals on the stream


def test_pose_only_composite_passes_only_its_tensors(ctx, gold, gold_preds):
    comp = metric.CompositeEvalMetric([metric.PointMatchingLossMetric(_cfg(), 0)])
    comp.update(None, {"point_matching_loss": gold_preds[0]["point_matching_loss"]})       # nothing else in preds
    host = comp._buf.asnumpy()
    assert host[3] != 0 and np.all(host[[0, 1, 2, 4]] == 0) and np.all(host[[5, 6, 7, 9]] == 0)


# ---- deepim_l2_norms_multi
def test_l2_norms_multi(ctx):
    rng = np.random.default_rng(77)
    lengths = [1, 3, 1023, 1024, 1025, 70001]
    host = [((rng.random(n) - 0.5) * 3.0).astype(np.float32) for n in lengths]
    dev = [odd_slice(ctx, a, 1 if i % 2 else 3) for i, a in enumerate(host)]
    assert any(d.ptr % 16 == 4 for d in dev) and all(d.ptr % 4 == 0 for d in dev)
    table = ctx.empty((len(dev), 2), np.uint64)
    table.copyfrom(np.array([[d.ptr, d.size] for d in dev], dtype=np.uint64))
    out = ctx.empty((len(dev),), np.float32)
    lib.deepim_l2_norms_multi(ctx.handle, out, table, len(dev))
    got = out.asnumpy()
    lib.deepim_l2_norms_multi(ctx.handle, out, table, len(dev))
    assert out.asnumpy().tobytes() == got.tobytes()
    for a, g in zip(host, got):
        want = float(np.sqrt(np.sum(a.astype(np.float64) ** 2)))
        print("n %6d: norm %.9g float64 %.17g relative %.3e" % (a.size, g, want, abs(g - want) / want))
        assert abs(float(g) - want) <= 1.2e-7 * want
    lib.deepim_l2_norms_multi(ctx.handle, out, table, 0)       # no rows: nothing to do

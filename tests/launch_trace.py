"""Host-only launch traces of the network graph (symbols/deepIM_flownet.py).

Everything the graph does on the device goes through `runtime.lib` and `DeviceArray`. `RecordingLib` stands in for `lib`: it
hands out fake addresses, answers the size / preferred / option queries with fixed values and records every other call. So
bind, one inference iteration and one training step run without a GPU, and the list of (entry, arguments) they produce pins
the launch order and every launch argument of a configuration. tests/test_launch_trace_host.py compares it with the golden
that tests/golden/make_launch_trace_golden.py wrote.
"""
import copy
import ctypes
import gc
import hashlib
import json
import sys
import weakref
import zlib

import numpy as np

from mx_deepim_amd import runtime
from mx_deepim_amd.config import default_config
from mx_deepim_amd.runtime import Context, DeviceArray

NUM_POINTS = 16
UNRECORDED = ("deepim_malloc", "deepim_free", "deepim_memset", "deepim_sync")
_BYREF = type(ctypes.byref(ctypes.c_int()))


class RecordingLib:
    """`load()` returns itself and every attribute is a recorder. `answers`: "preferred" (every *_preferred* / *_supported
    query), "wgrad_lds" (deepim_get_option) and "weight_order" (deepim_conv_weight_order)."""

    def __init__(self, preferred=1, wgrad_lds=1, weight_order=2):
        self.answers = {"preferred": preferred, "wgrad_lds": wgrad_lds, "weight_order": weight_order}
        self.calls = []          # (entry, raw arguments): pointers are resolved to names by Tracer.take()
        self.allocs = []         # (address, bytes), ascending and never reused
        self._next = 1 << 32
        self._handles = 0
        self.observer = None     # called with the frozen arguments of every recorded call

    def load(self):
        return self

    def last_error(self):
        return ""

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def entry(*args):
            return self._call(name, args)

        entry.__name__ = name
        return entry

    def _call(self, name, args):
        if name == "deepim_create":
            self._handles += 1
            args[1]._obj.value = self._handles
            return 0
        if name == "deepim_malloc":
            nbytes = int(args[1])
            args[2]._obj.value = self._next
            self.allocs.append((self._next, nbytes))
            self._next += (nbytes + 511) // 256 * 256
            return 0
        if name in UNRECORDED:
            return 0
        self.calls.append((name, tuple(_freeze(a) for a in args)))
        if self.observer is not None:
            self.observer(self.calls[-1][1])
        if name.endswith("_size"):
            # a fixed function of the arguments, a multiple of 16 bytes
            return 256 + 16 * (sum((i + 1) * int(a) for i, a in enumerate(args) if isinstance(a, (int, np.integer))) % 4093)
        if "_preferred" in name or name.endswith("_supported"):
            return self.answers["preferred"]
        if name == "deepim_conv_weight_order":
            return self.answers["weight_order"]
        if name == "deepim_get_option":
            args[2]._obj.value = self.answers[args[1].decode()]
        return 0


def _freeze(a):
    """One raw argument in a form that outlives the call: ("ptr", address), ("host", bytes if small, dtype, shape, checksum) or a
    plain value."""
    if isinstance(a, DeviceArray):
        return ("ptr", a.ptr)
    if isinstance(a, np.ndarray):
        return ("host", a.tobytes() if a.nbytes <= 1 << 16 else None, str(a.dtype), a.shape, zlib.crc32(a))
    if isinstance(a, ctypes.c_void_p):
        return ("ctx", a.value)
    if isinstance(a, _BYREF):
        return ("byref",)
    if isinstance(a, (ctypes.c_float, ctypes.c_double, ctypes.c_int)):
        return a.value
    if isinstance(a, bytes):
        return a.decode()
    if isinstance(a, (bool, np.bool_)):
        return int(a)
    if isinstance(a, np.integer):
        return int(a)
    if isinstance(a, np.floating):
        return float(a)
    assert a is None or isinstance(a, (int, float)), (type(a), a)
    return a


def install(fake, setattr_):
    """Put `fake` in the place of `lib` in the runtime and in every loaded symbols module (`setattr_`: monkeypatch.setattr).
    Fake arrays must never reach the real deepim_free: their finaliser is switched off for as long as the patch holds, and
    `trace_config` disowns and collects every array made under it before it returns. -> the weak references of those arrays."""
    made, init = [], DeviceArray.__init__

    def tracked_init(self, *a, **kw):
        init(self, *a, **kw)
        made.append(weakref.ref(self))

    setattr_(DeviceArray, "__init__", tracked_init)
    setattr_(runtime, "lib", fake)
    for modname, mod in list(sys.modules.items()):
        if modname.startswith("mx_deepim_amd.symbols.") and hasattr(mod, "lib"):
            setattr_(mod, "lib", fake)
    setattr_(DeviceArray, "__del__", lambda self: None)
    return made


class Tracer:
    """Resolves the raw calls of a RecordingLib into the trace: buffers by the name under which the network or the batch holds
    them."""

    CONTAINERS = ("params", "packed", "packed_wino", "wino_s2d3", "packed_wino_dgrad", "packed_f16", "packed_f16_wino", "packed_x3",
                  "packed_dec16", "act", "ws", "grad", "mom", "adam_mean", "adam_var")
    SINGLE = ("wino_conv1", "amp_state", "opt_state")
    TABLES = ("_sgd_table", "_adam_table")

    def __init__(self, fake, net, batch):
        self.fake, self.net, self.batch, self.done = fake, net, batch, 0
        self.names = {}          # address → name; a name, once given, stays (a buffer may be dropped later, as bind_train drops
        fake.observer = self._observe     # the rot / trans weights of bind for rows of one shared buffer)

    def _observe(self, args):
        if any(isinstance(a, tuple) and a[0] == "ptr" and a[1] not in self.names for a in args):
            self._names()

    def _names(self):
        """Names for the buffers the network and the batch hold now: the first holder in a fixed order wins."""
        exact = self.names

        def put(name, a):
            if isinstance(a, DeviceArray):
                exact.setdefault(a.ptr, name)

        for attr in self.CONTAINERS:
            d = getattr(self.net, attr, None)
            if isinstance(d, dict):
                for k in d:
                    put("%s.%s" % (attr, k), dict.__getitem__(d, k))
        for k, (raw, _co, _ci, _khw) in getattr(getattr(self.net, "grad", None), "tm", {}).items():
            put("grad.tm.%s" % k, raw)
        for attr in self.SINGLE:
            put(attr, getattr(self.net, attr, None))
        for attr in self.TABLES:
            tab = getattr(self.net, attr, None)
            if tab is not None:
                put(attr, tab[1])
        for group, d in self.batch.items():
            for k, a in d.items():
                put("%s.%s" % (group, k), a)
        return exact

    def _resolve(self, ptr, exact):
        if ptr in exact:
            return exact[ptr]
        for base, nbytes in self.fake.allocs:       # a view: the allocation's holder plus the byte offset
            if base <= ptr < base + max(nbytes, 1) and base in exact:
                return "%s+%d" % (exact[base], ptr - base)
        raise LookupError("device pointer %#x is held under no name" % ptr)

    def take(self):
        """The calls recorded since the last take(), resolved. Call it at the end of a phase, when every buffer is stored."""
        exact = self._names()
        out = []
        for name, args in self.fake.calls[self.done:]:
            res = []
            for a in args:
                if isinstance(a, tuple) and a[0] == "ptr":
                    res.append(self._resolve(a[1], exact))
                elif isinstance(a, tuple) and a[0] == "host":
                    res.append("host:%s:%08x" % (a[2], a[4]))
                elif isinstance(a, tuple) and a[0] == "ctx":
                    res.append("ctx%d" % a[1])
                elif isinstance(a, tuple):
                    res.append(a[0])
                else:
                    res.append(a)
            if name == "deepim_h2d" and res[1] in self.TABLES:
                # the optimizer's pointer table: rows {w, *states, g, n, wd | block << 32, layout} with the pointers as names
                host = [a for a in args if isinstance(a, tuple) and a[0] == "host"][0]
                rows = np.frombuffer(host[1], np.uint64).reshape(host[3])
                nptr = rows.shape[1] - 3
                res[2] = [[self._resolve(int(v), exact) for v in r[:nptr]] + [int(v) for v in r[nptr:]] for r in rows]
            out.append([name] + res)
        self.done = len(self.fake.calls)
        return out


def _pattern(shape, salt):
    """A fixed, generator-free host tensor in (-0.05, 0.05)."""
    n = int(np.prod(shape))
    v = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(977 * salt + 1)) % np.uint64(2001)).astype(np.float32)
    return ((v - 1000.0) * np.float32(5e-5)).reshape(shape)


_PARAMS = {}


def host_params(net):
    """name → host tensor for every parameter of the graph, cached per shape (fc6 is 84 MB)."""
    out = {}
    for salt, (name, shape) in enumerate(sorted(net.arg_shape_dict().items())):
        key = (name, tuple(shape))
        if key not in _PARAMS:
            _PARAMS[key] = _pattern(shape, salt)
        out[name] = _PARAMS[key]
    return out


def _cfg(network=(), test=(), train=(), train_iter=()):
    cfg = copy.deepcopy(default_config())
    for sect, kv in (("network", network), ("TEST", test), ("TRAIN", train), ("train_iter", train_iter)):
        cfg[sect].update(dict(kv))
    return cfg


# name → (training graph?, batch, config overrides, lib answers, attributes set on the net after bind)
CONFIGS = {
    "test_default": (False, 2, {}, {}, {}),
    "test_full": (False, 2, {"test": {"FAST_TEST": False}}, {}, {}),
    "test_fp16_full_dec16": (False, 2, {"network": {"FP16_CONV": True}, "test": {"FAST_TEST": False}}, {}, {}),
    "test_fp16_full_dec32": (False, 2, {"network": {"FP16_CONV": True, "FP16_DECODER": False}, "test": {"FAST_TEST": False}}, {}, {}),
    "test_fp16_wino": (False, 2, {"network": {"FP16_CONV": True, "FP16_WINOGRAD": True}}, {}, {}),
    "test_fp16_depth": (False, 2, {"network": {"FP16_CONV": True, "INPUT_DEPTH": True}}, {}, {}),
    "test_x3": (False, 2, {"network": {"X3_CONV": True}}, {}, {}),
    "test_euler": (False, 2, {"network": {"ROT_TYPE": "EULER"}}, {}, {}),
    "test_no_mask": (False, 2, {"network": {"INPUT_MASK": False}}, {}, {}),
    "test_nchw": (False, 2, {"network": {"NC8_CONV": False}}, {}, {}),
    "test_not_preferred": (False, 2, {}, {"preferred": 0}, {}),
    "test_conv1_nc8": (False, 2, {}, {}, {"conv1_nc8": True}),
    "train_default": (True, 2, {}, {}, {}),
    "train_default_b8": (True, 8, {}, {}, {}),
    "train_no_wgrad_lds": (True, 2, {}, {"wgrad_lds": 0}, {}),
    "train_pose_only": (True, 2, {"network": {"PRED_FLOW": False, "PRED_MASK": False}}, {}, {}),
    "train_se3_dist": (True, 2, {"train_iter": {"SE3_DIST_LOSS": True, "LW_ROT": 1.0, "LW_TRANS": 1.0}}, {}, {}),
    "train_wino": (True, 2, {"train": {"WINOGRAD_CONV": True}}, {}, {}),
    "train_wino_not_preferred": (True, 2, {"train": {"WINOGRAD_CONV": True}}, {"preferred": 0}, {}),
    "train_fp16": (True, 2, {"network": {"FP16_CONV": True}}, {}, {}),
    "train_x3": (True, 2, {"train": {"X3_CONV": True}}, {}, {}),
    "train_adam": (True, 2, {"train": {"optimizer": "adam"}}, {}, {}),
}

DATA_KEYS = ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "depth_observed", "depth_rendered", "src_pose")
LABEL_KEYS = ("mask_gt_observed", "point_cloud_model", "point_cloud_weights", "point_cloud_observed", "flow", "flow_weights",
              "rot", "trans")


def trace_config(name, setattr_):
    """{phase: trace} of configuration `name`, run on a RecordingLib installed through `setattr_` (monkeypatch.setattr)."""
    from mx_deepim_amd.symbols import deepIM_flownet

    is_train, B, over, answers, attrs = CONFIGS[name]
    fake = RecordingLib(**answers)
    made = install(fake, setattr_)
    try:
        ctx = Context(0)
        Context.opened.pop()
        net = deepIM_flownet().get_symbol(_cfg(**over), is_train=is_train)
        batch = {"data": {k: ctx.empty((B, 4)) for k in DATA_KEYS}, "label": {k: ctx.empty((B, 4)) for k in LABEL_KEYS}}
        tracer = Tracer(fake, net, batch)
        tracer.take()
        out = {}
        if is_train:
            net.bind_train(ctx, B, host_params(net), num_points=NUM_POINTS)
            out["bind_train"] = tracer.take()
            net.forward_train(batch["data"], batch["label"])
            net.backward()
            net.update(1e-4)
            out["step"] = tracer.take()
        else:
            net.bind(ctx, B, host_params(net))
            out["bind"] = tracer.take()
            for k, v in attrs.items():
                setattr(net, k, v)
            net.refine_iteration(batch["data"])
            out["refine_iteration"] = tracer.take()
        return out
    finally:
        for ref in made:      # whatever outlives the patch must not hand a fake address to the real deepim_free
            if ref() is not None:
                ref()._owner = False
        fake.observer = net = batch = tracer = None
        gc.collect()      # while the finaliser is still switched off


def normalise(trace):
    """A run of consecutive *pack_weights* calls as a sorted run: those launches are independent of each other on one stream, so
    their relative order carries no behaviour. Everything else stays in call order."""
    out, run = [], []
    for call in trace:
        if "pack_weights" in call[0]:
            run.append(json.dumps(call))
            continue
        out += sorted(run) + [json.dumps(call)]
        run = []
    return out + sorted(run)


def digest(trace):
    return hashlib.sha256("\n".join(normalise(trace)).encode()).hexdigest()

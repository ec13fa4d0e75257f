"""§8f-4d — fp32 Winograd training (TRAIN.WINOGRAD_CONV), the parts that need no GPU: the config key and what the training symbol
makes of it, the new C entry points in the header, and the identity the Winograd data gradient rests on: the data gradient of a 3x3
stride-1 pad-1 convolution is the F(2x2,3x3) Winograd convolution of dz with the transposed, flipped weights."""
import numpy as np
import pytest

from oracle import net as onet
from oracle import wino as owino
from mx_deepim_amd import runtime
from mx_deepim_amd.config import default_config
from mx_deepim_amd.symbols import deepIM_flownet

NEW_ENTRIES = ("deepim_lrelu_bias_backward_nc8", "deepim_conv2d_wgrad_tm_nc8", "deepim_conv_wino_pack_weights_dgrad",
               "deepim_conv2d_wino_dgrad")


def test_the_key_defaults_to_off_and_the_training_symbol_follows_it():
    cfg = default_config()
    assert cfg.TRAIN.WINOGRAD_CONV is False
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    assert net.nc8 is False and net.train_winograd is False
    cfg = default_config()
    cfg.TRAIN.WINOGRAD_CONV = True
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    assert net.nc8 is True and net.train_winograd is True
    cfg = default_config()
    cfg.TRAIN.WINOGRAD_CONV = True
    cfg.network.FP16_CONV = True          # the fp16 graph ignores the key
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    assert net.nc8 is False and net.train_winograd is False
    # the inference symbol is not touched by it
    cfg = default_config()
    cfg.TRAIN.WINOGRAD_CONV = True
    assert deepIM_flownet().get_symbol(cfg).nc8 is True and deepIM_flownet().get_symbol(default_config()).nc8 is True


def test_the_new_entry_points_are_declared():
    protos = runtime.parse_header()
    for name in NEW_ENTRIES:
        assert name in protos, name
    assert protos["deepim_lrelu_bias_backward_nc8"][2] == ["ctx", "dz", "dz_nc8", "db", "dy", "add", "y_nc8", "y_mode", "slope", "B", "C",
                                                           "H", "W"]
    assert protos["deepim_conv2d_wgrad_tm_nc8"][2] == ["ctx", "dw_tm", "x_nc8", "x_mode", "dz", "B", "Cin", "H", "W", "Cout", "kh", "kw",
                                                       "stride", "pad"]
    assert protos["deepim_conv2d_wino_dgrad"][2] == ["ctx", "dx", "dz_nc8", "packed_w", "B", "Cin", "H", "W", "Cout"]
    assert protos["deepim_conv_wino_pack_weights_dgrad"][2] == ["ctx", "packed_w", "w", "Cout", "Cin"]


# (B, Cin, H, W, Cout) of the layer whose data gradient is taken
DGRAD_CASES = [(2, 256, 16, 20, 256), (2, 512, 15, 20, 512), (2, 1024, 8, 10, 1024), (1, 64, 30, 40, 128)]


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_data_gradient_is_the_winograd_convolution_with_transposed_flipped_weights(case):
    """dx = winograd_f2x2_3x3(dz, w^T flipped) against the oracle's float64 data gradient. float64 transforms: the difference is the
    oracle's own float32 rounding of dx (<= 4.8e-8 of the range measured on these cases), bar 1e-6. float32 transforms (the kernel's
    arithmetic): 5.4e-7 … 1.24e-6 measured, bar 1e-5 of the range (the Winograd bar of DESIGN.md §4)."""
    B, cin, H, W, cout = case
    rng = np.random.default_rng(sum(case))
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    dz = rng.standard_normal((B, cout, H, W)).astype(np.float32)
    x = np.zeros((B, cin, H, W), np.float32)
    ref = np.asarray(onet.conv2d_backward(x, w, dz, 1, 1)[0], np.float64)
    wt = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
    scale = float(np.abs(ref).max())
    for dtype, bar in ((np.float64, 1e-6), (np.float32, 1e-5)):
        got = np.asarray(owino.winograd_f2x2_3x3(dz, wt, dtype=dtype), np.float64)[:, :, :H, :W]
        err = float(np.abs(got - ref).max()) / scale
        print("case %s %s: %.3g of the range" % (case, np.dtype(dtype).name, err))
        assert got.shape == ref.shape
        assert err <= bar, (case, dtype, err)

"""CPU suite of the dynamic loss scale of the fp16 matrix path: the library plans a non-saturating launch (gim_conv_shape.prec = 2)
exactly like a saturating one, and ops.set_loss_scale validates what it is given.  (What the kernels and the guarded Adam step
compute is a GPU matter: tests/test_gpu_loss_scaler.py.)"""
import ctypes
import math
import warnings

import pytest

from tests.test_gpu_fp16 import PLAIN


def _plan(lib, sh, kind):
    out = (ctypes.c_int32 * 8)()
    rc = lib.gim_conv_launch_plan(ctypes.byref(sh), kind, ctypes.cast(out, ctypes.c_void_p))
    return rc, list(out)


@pytest.mark.parametrize("case", PLAIN, ids=[str(c) for c in PLAIN])
def test_prec2_takes_the_launch_plan_of_prec1(case):
    from optimalstrategiesagainstgenerativeattacks_amd import _lib, ops
    lib = _lib.load()
    N, Cin, Cout, K, H, slope, _ = case
    prev = ops.set_matrix_path("fp16")
    try:
        sh = ops._shape(N, H, H, Cin, Cout, K, 0, slope)
    finally:
        ops.set_matrix_path(prev)
    assert sh.prec == 1
    for kind in (0, 2, 3):
        sh.prec = 1
        rc1, plan1 = _plan(lib, sh, kind)
        sh.prec = 2
        rc2, plan2 = _plan(lib, sh, kind)
        assert rc1 == 0 and rc2 == 0, (kind, rc1, rc2, lib.gim_last_error())
        assert plan1 == plan2 and plan1[7] & 255 == 2, (kind, plan1, plan2)
        sh.prec = 3
        assert _plan(lib, sh, kind)[0] != 0, "prec = 3 must be refused"


def test_armed_backward_selects_prec2_on_the_fp16_path_only():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    args = (2, 8, 8, 32, 64, 3, 0, 0.2)
    assert ops._shape(*args).prec == 0
    with ops.armed_backward(object()):
        assert ops._shape(*args).prec == 0          # fp32 path: nothing to arm
    prev = ops.set_matrix_path("fp16")
    try:
        assert ops._shape(*args).prec == 1
        with ops.armed_backward(object()):
            assert ops._shape(*args).prec == 2
            assert ops._shape(2, 1, 1, 32, 64, 1, 0, 1.0).prec == 0   # linears stay fp32
        with ops.armed_backward(None):
            assert ops._shape(*args).prec == 1      # no scaler: not armed
        assert ops._shape(*args).prec == 1          # the template cache keeps the two apart
    finally:
        ops.set_matrix_path(prev)


def test_set_loss_scale_validates_and_switches_the_mode():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    assert ops.matrix_path() == "fp32" and ops.loss_scale() == 1.0
    start = ops.set_loss_scale(4096)
    try:
        for bad in (0, -4, "abc", float("nan"), "nan", None):
            with pytest.raises(ValueError):
                ops.set_loss_scale(bad)
        assert ops.loss_scale_mode() == "static"
        with pytest.warns(UserWarning, match="power of two"):
            assert ops.set_loss_scale(3000) == 4096.0
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert ops.set_loss_scale(3000) == 3000.0          # warned once
            assert ops.set_loss_scale(2.0 ** -3) == 3000.0     # powers of two: no warning
            assert ops.set_loss_scale("1024") == 0.125
        assert ops.set_loss_scale("dynamic", init=2048, growth_interval=7, min_scale=2.0) == 1024.0
        assert ops.loss_scale_mode() == "dynamic"
        assert ops.dynamic_loss_scale_defaults() == {"init": 2048.0, "growth_interval": 7, "min_scale": 2.0}
        assert ops.loss_scale() == 1.0                         # still 1 on the fp32 path
        prev = ops.set_matrix_path("fp16")
        try:
            assert ops.loss_scale() == 2048.0
        finally:
            ops.set_matrix_path(prev)
        for kw in (dict(init=0), dict(min_scale=-1.0), dict(growth_interval=0)):
            with pytest.raises(ValueError):
                ops.set_loss_scale("dynamic", **kw)
        assert ops.set_loss_scale("dynamic") == "dynamic"
        d = ops.dynamic_loss_scale_defaults()
        assert d == {"init": 4096.0, "growth_interval": 2000, "min_scale": 1.0}
        assert ops.set_loss_scale(512) == "dynamic" and ops.loss_scale_mode() == "static"
    finally:
        ops.set_loss_scale(start)
    assert ops.loss_scale() == 1.0


def test_growth_interval_default_is_torch_amp_grad_scalers():
    import inspect
    import torch
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    ref = inspect.signature(torch.amp.GradScaler.__init__).parameters["growth_interval"].default
    assert inspect.signature(ops.set_loss_scale).parameters["growth_interval"].default == ref == 2000
    assert math.frexp(inspect.signature(ops.set_loss_scale).parameters["init"].default)[0] == 0.5

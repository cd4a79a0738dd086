"""The learning-rate schedule and the device-word Adam entry points, as far as they can be checked without a device:
`optim.StepLR` against `torch.optim.lr_scheduler.StepLR` (exact floats), the fp32 the device word receives against the fp32 a
by-value `float` argument receives, the argument checks of sn2_adam_step_dev / sn2_adam_step_images_dev, and the meter's size
constant against the header."""
import ctypes
import os
import re
import warnings
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from stratanet2_vegetation_coverage_maps_amd.optim import StepLR

SETTINGS = [(1, 0.75), (3, 0.5), (50, 0.1), (2, 0.9)]          # (step_size, gamma); the first is main_SSL.py's default
EPOCHS = 200
LR0 = 1e-3


def _torch_schedule(step_size, gamma, epochs=EPOCHS, lr0=LR0):
    """[lr after epoch 1, 2, ...] of torch's StepLR over a dummy CPU optimiser, as Python floats."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr0)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=step_size, gamma=gamma)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # (scheduler stepped without optimizer.step(): no update is meant)
        for _ in range(epochs):
            sched.step()
            out.append((opt.param_groups[0]["lr"], sched.get_last_lr()[0], sched.last_epoch))
    return out


@pytest.mark.parametrize("step_size,gamma", SETTINGS)
def test_step_lr_reproduces_torch_exactly(step_size, gamma):
    ref = _torch_schedule(step_size, gamma)
    holder = SimpleNamespace(lr=LR0)                             # anything with an `lr` attribute
    sched = StepLR(holder, step_size, gamma)
    assert sched.last_epoch == 0 and sched.get_last_lr() == [LR0]
    for e, (lr, last, epoch) in enumerate(ref):
        sched.step()
        assert holder.lr == lr, f"epoch {e + 1}: {holder.lr!r} != torch's {lr!r}"
        assert sched.get_last_lr() == [last] and sched.last_epoch == epoch
    assert ref[-1][0] < LR0, "the schedule under test never moved"


@pytest.mark.parametrize("step_size,gamma", SETTINGS)
def test_step_lr_state_dict_round_trip_in_mid_schedule(step_size, gamma):
    ref = _torch_schedule(step_size, gamma)
    cut = 77                                                     # in mid-period for step sizes 2, 3 and 50
    a = SimpleNamespace(lr=LR0)
    sa = StepLR(a, step_size, gamma)
    for _ in range(cut):
        sa.step()
    saved, saved_lr = sa.state_dict(), a.lr
    b = SimpleNamespace(lr=saved_lr)                             # the rate is the optimiser's state (FlatAdam.state_dict()["lr"])
    sb = StepLR(b, 1, 0.123)
    sb.load_state_dict(saved)
    assert sb.state_dict() == saved and sb.get_last_lr() == [ref[cut - 1][0]]
    for e in range(cut, EPOCHS):
        sb.step()
        assert b.lr == ref[e][0] and sb.last_epoch == ref[e][2]


def test_step_lr_refuses_a_step_size_below_one():
    with pytest.raises(ValueError):
        StepLR(SimpleNamespace(lr=LR0), 0, 0.5)


def test_fp32_fill_equals_the_by_value_float_conversion():
    """`FlatAdam.lr = x` is `lr_dev.fill_(x)` on an fp32 tensor; sn2_adam_step takes `x` through ctypes' c_float.  Both must
    round the schedule's Python floats to the same fp32, else the device-word path trains with another rate than the by-value
    one did."""
    word = torch.empty(1, dtype=torch.float32)
    seen = 0
    for step_size, gamma in SETTINGS:
        for lr, _, _ in _torch_schedule(step_size, gamma):
            word.fill_(lr)
            assert word.item() == ctypes.c_float(lr).value, f"{lr!r}"
            seen += 1
    for lr in (LR0, 0.0, 1e-45, 1.0 + 2.0 ** -24, 3.4e38):        # denormal result, a tie, near the top
        word.fill_(lr)
        assert word.item() == ctypes.c_float(lr).value, f"{lr!r}"
    assert seen == len(SETTINGS) * EPOCHS


def test_meter_terms_constant_matches_the_header():
    from stratanet2_vegetation_coverage_maps_amd import _lib
    txt = open(os.path.join(ROOT, "include", "strata_hip.h")).read()
    m = re.search(r"^#define\s+SN2_METER_TERMS\s+(\d+)\s*$", txt, flags=re.M)
    assert m is not None, "SN2_METER_TERMS is not defined in strata_hip.h"
    assert _lib.SN2_METER_TERMS == int(m.group(1)) == _lib.CONSTANTS["SN2_METER_TERMS"] == 4


def test_dev_entry_points_check_their_arguments_before_any_device_work():
    """sn2_adam_step_dev / sn2_adam_step_images_dev return SN2_EINVAL (-1) without touching a device for: a NULL lr_dev, n_terms
    outside 0 .. SN2_METER_TERMS, n_terms > 0 with terms or meter NULL -- and for everything their by-value siblings refuse.  The
    pointers are fake and never dereferenced: every call below fails a check first."""
    from stratanet2_vegetation_coverage_maps_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    lib = _lib.load()
    fake, n = 0x1000, 257
    hyper = (0.9, 0.999, 1e-8, 1e-3)

    def plain(param=fake, grad=fake, m=fake, v=fake, n=n, lr_dev=fake, step=fake, terms=fake, n_terms=4, meter=fake):
        return lib.sn2_adam_step_dev(param, grad, m, v, n, lr_dev, *hyper, step, 1.0, terms, n_terms, meter, None)

    def images(param=fake, arena=fake, replicas=32, stride=320, m=fake, v=fake, n=n, lr_dev=fake, step=fake, terms=fake, n_terms=4,
               meter=fake):
        return lib.sn2_adam_step_images_dev(param, arena, replicas, stride, m, v, n, lr_dev, *hyper, step, 1.0, terms, n_terms, meter,
                                            None)

    for fn in (plain, images):
        assert fn(lr_dev=None) == -1, "NULL lr_dev"
        assert fn(lr_dev=None, terms=None, n_terms=0, meter=None) == -1, "NULL lr_dev without a meter"
        assert fn(n_terms=-1) == -1 and fn(n_terms=_lib.SN2_METER_TERMS + 1) == -1, "n_terms out of range"
        for k in range(1, _lib.SN2_METER_TERMS + 1):
            assert fn(n_terms=k, terms=None) == -1, f"{k} terms from a NULL buffer"
            assert fn(n_terms=k, meter=None) == -1, f"{k} terms into a NULL meter"
        # the existing checks still apply (with otherwise valid new arguments)
        assert fn(param=None) == -1 and fn(m=None) == -1 and fn(v=None) == -1 and fn(step=None) == -1
        assert fn(n=0) == -1 and fn(n=-5) == -1
    assert plain(grad=None) == -1
    assert images(arena=None) == -1 and images(replicas=0) == -1 and images(replicas=2, stride=n - 1) == -1

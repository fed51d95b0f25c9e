"""Optimistic Adam, the parts that need no GPU: the C entry is declared alike in the header and in _lib's signature table (test_host's
export test then covers the shared library), FusedAdam.enable_optimism checks omega before any GPU work, the trainers take the new
arguments, and the fp64 restatement of the rule (tests/oadam_ref.py, the reference of the GPU tests) does on a bilinear game what
the rule is for."""
import inspect
import os
import re

import pytest
import torch

from tests import oadam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opt():
    from optimalstrategiesagainstgenerativeattacks_amd.optim import FusedAdam
    return FusedAdam([torch.nn.Parameter(torch.zeros(7))], lr=1e-3)


def test_header_and_signature_table_agree_on_fifteen_arguments():
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    header = open(os.path.join(ROOT, "include", "gim_hip.h")).read()
    found = re.search(r"^int gim_adam_optimism\(([^)]*)\);", header, re.M)
    assert found, "gim_hip.h does not declare gim_adam_optimism"
    args = [" ".join(a.split()) for a in found.group(1).split(",")]
    assert args == ["float* p", "float* prev", "const float* m", "const float* v", "int64_t n", "const int64_t* seg_end", "const float* lr",
                    "int n_seg", "float beta1", "float beta2", "float eps", "float omega", "const int32_t* step",
                    "const void* scaler_state", "void* stream"], args
    sig = _lib.SIGNATURES["gim_adam_optimism"]
    assert len(sig) == len(args) == 15
    P, I64, I, F = _lib.SIGNATURES["gim_ema_update"][0], _lib.SIGNATURES["gim_ema_update"][2], _lib.SIGNATURES["gim_adam_step"][7], \
        _lib.SIGNATURES["gim_ema_update"][3]
    for a, c in zip(args, sig):
        want = P if "*" in a else {"int64_t": I64, "int": I, "float": F}[a.split()[0]]
        assert c is want, (a, c)


@pytest.mark.parametrize("omega", [0.0, -0.5, 1.5, float("nan"), 1.0 + 1e-6, float("inf")])
def test_enable_optimism_rejects_omega_outside_the_half_open_unit_interval(omega):
    opt = _opt()
    with pytest.raises(ValueError):
        opt.enable_optimism(omega)
    assert opt.optimism is None and opt.flat_prev is None


@pytest.mark.parametrize("omega", [1.0, 0.5, 1e-3, 1.0 + 1e-9])      # the last rounds to 1.0f: the float32 value decides
def test_enable_optimism_accepts_and_reports_omega(omega):
    opt = _opt()
    assert opt.optimism is None
    opt.enable_optimism(omega)
    assert opt.optimism == omega
    assert opt.flat_prev is None, "nothing is allocated before the build"
    opt.disable_optimism()
    assert opt.optimism is None


def test_optimism_accessors_need_the_switch():
    opt = _opt()
    for call in (opt.optimism_state, opt.prime_optimism, lambda: opt.load_optimism({})):
        with pytest.raises(RuntimeError, match="enable_optimism"):
            call()


def test_trainers_take_omega_as_keyword_arguments_in_front_of_the_decays():
    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd.gim_gaussian_trainer import GIMGaussianTrainer
    from optimalstrategiesagainstgenerativeattacks_amd.gim_img_training import train_gim_imgs
    for fn in (G.GIMImgTrainer.__init__, GIMGaussianTrainer.__init__, train_gim_imgs):
        ps = list(inspect.signature(fn).parameters.values())[-4:]
        assert [(p.name, p.default) for p in ps] == [("im_optimism", None), ("au_optimism", None), ("im_ema_decay", None),
                                                     ("au_ema_decay", None)], fn


def test_bilinear_game_in_fp64():
    """64-dimensional x^T y, Adam (0, 0.99), lr 3e-2, 1000 simultaneous steps, seed 0.  Over seeds 0-19 the restatement gives
    0.575-0.678 without and 0.055-0.123 with the optimistic step, so both conditions have room."""
    plain, half, optimistic = (ref.bilinear_game(0, w) for w in (0.0, 0.5, 1.0))
    print("bilinear game, seed 0: final / start distance %.4f (omega 0)  %.4f (0.5)  %.4f (1)" % (plain, half, optimistic))
    assert plain >= 0.45, plain
    assert optimistic <= 0.25, optimistic
    assert optimistic < half < plain

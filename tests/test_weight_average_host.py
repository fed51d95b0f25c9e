"""Averaged agents, the parts that need no GPU: the decay check of FusedAdam.enable_averaging runs before any GPU work, and the two
C entries (gim_ema_update, gim_buffer_exchange) are declared in the header and in _lib's signature table (test_host's export test
then covers the shared library)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opt():
    from optimalstrategiesagainstgenerativeattacks_amd.optim import FusedAdam
    return FusedAdam([torch.nn.Parameter(torch.zeros(7))], lr=1e-3)


@pytest.mark.parametrize("decay", [1.0, -0.1, 1.5, float("nan")])
def test_enable_averaging_rejects_decays_outside_the_half_open_unit_interval(decay):
    opt = _opt()
    with pytest.raises(ValueError):
        opt.enable_averaging(decay)
    assert opt.averaging is None


@pytest.mark.parametrize("decay", [0.0, 0.999])
def test_enable_averaging_accepts_and_reports_the_decay(decay):
    opt = _opt()
    assert opt.averaging is None
    opt.enable_averaging(decay)
    assert opt.averaging == decay
    opt.disable_averaging()
    assert opt.averaging is None


def test_signature_table_has_both_entries():
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    assert len(_lib.SIGNATURES["gim_ema_update"]) == 6
    assert len(_lib.SIGNATURES["gim_buffer_exchange"]) == 4


def test_header_declares_both_entries():
    header = open(os.path.join(ROOT, "include", "gim_hip.h")).read()
    assert re.search(r"^int gim_ema_update\(float\* avg, const float\* p, int64_t n, float decay, const void\* scaler_state, void\* stream\);",
                     header, re.M)
    assert re.search(r"^int gim_buffer_exchange\(float\* a, float\* b, int64_t n, void\* stream\);", header, re.M)


def test_trainers_take_the_decays_as_last_keyword_arguments():
    import inspect

    import optimalstrategiesagainstgenerativeattacks_amd as G
    from optimalstrategiesagainstgenerativeattacks_amd.gim_gaussian_trainer import GIMGaussianTrainer
    from optimalstrategiesagainstgenerativeattacks_amd.gim_img_training import train_gim_imgs
    for fn in (G.GIMImgTrainer.__init__, GIMGaussianTrainer.__init__, train_gim_imgs):
        ps = list(inspect.signature(fn).parameters.values())[-2:]
        assert [(p.name, p.default) for p in ps] == [("im_ema_decay", None), ("au_ema_decay", None)], fn

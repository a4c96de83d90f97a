"""The conv-family engine calls of the networks and of one trainer step against tests/golden/conv_calls.json.gz (tests/conv_calls.py):
same entry points in the same order with the same arguments.  The fixture was recorded on the commit before cc_amd/ops.py got its
launchers and ops.conv2d became the one-member case of the group Function, so the sequences are the ones the hand-written call
sites made.  `tape` and `step` are compared as logged; `layers` (the per-layer path) in group spelling, see
conv_calls.group_spelling."""
import pytest

import conv_calls as CC
from oracle.make_golden import ALT_NETS


@pytest.fixture(scope="module")
def want():
    return CC.load_fixture()


def _same(got, want, key):
    got = CC.plain(got)
    assert [c[0] for c in got] == [c[0] for c in want[key]], key
    for k, (a, b) in enumerate(zip(got, want[key])):
        assert a == b, (key, k, a, b)


def _tape(dev, want, name):
    _same(CC.trace_tape(dev, name)[1], want, "tape." + name)


def _layers(dev, want, name):
    calls = CC.trace_config1(dev)[1] if name == "config1" else CC.trace_alt(dev, name, dict(ALT_NETS)[name])[1]
    _same(CC.group_spelling(calls), want, "layers." + name)


LAYERS = [n for n, _ in ALT_NETS] + ["config1"]


@pytest.mark.parametrize("name", list(CC.TAPE_NETS))
def test_tape_calls_emulated(want, name):
    from hipemu.emu import emulated_engine
    with emulated_engine():
        _tape("cpu", want, name)


@pytest.mark.slow
def test_step_calls_emulated(want):
    from hipemu.emu import emulated_engine
    with emulated_engine():
        _same(CC.trace_step("cpu")[1], want, "step")


@pytest.mark.parametrize("name", LAYERS)
def test_layers_calls_emulated(want, name):
    from hipemu.emu import emulated_engine
    with emulated_engine():
        _layers("cpu", want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CC.TAPE_NETS))
def test_tape_calls_gpu(want, name):
    _tape("cuda", want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYERS)
def test_layers_calls_gpu(want, name):
    _layers("cuda", want, name)


def test_parked_bias_sum_is_reduced_before_its_target_is_parked_again_emulated():
    """ops._act_bwd_bias inside a stage (queue enabled, accumulate): the second stage of a bias sum is parked; a second call on the
    SAME bias first runs what is parked (two parked `gb +=` of one target would race in one reduce table).  2 x 2 x 128 x 160: above
    the B * H * W <= 32768 bound under which the kernel writes the bias gradient itself and nothing is parked."""
    import torch
    from cc_amd import ops
    from cc_amd.step_scope import StepScope
    from hipemu.emu import emulated_engine
    gen = torch.Generator().manual_seed(7)
    gy, y = torch.randn(2, 2, 128, 160, generator=gen), torch.randn(2, 2, 128, 160, generator=gen)
    gb = torch.zeros(2)
    ge = [torch.empty_like(gy) for _ in range(2)]
    with emulated_engine():
        with StepScope() as scope, CC.ConvLog() as log:
            scope.park_weight_gradients()
            for k in range(2):
                ops._act_bwd_bias([gy], [y], [ge[k]], [gb], 1, 1.0, 0.0, True)
            ops.wgrad_reduces.flush()
    got = [(c[0], c[1][1]) if c[0] == "cc_wgrad_reduce_table" else c[0] for c in log.calls if not c[0].endswith("_ws_bytes")]
    assert got == ["cc_act_bwd_bias_group_defer", ("cc_wgrad_reduce_table", 1)] * 2, got
    # both calls added sum over (n, h, w) of gy * relu'(y): fp32 sums of 81920 terms per channel, summed in lanes, trees and chunks,
    # no chain of additions longer than 64 -> |error| <= 64 * 2^-24 * sum |term| (first-order bound of recursive summation)
    terms = (gy * (y > 0)).double()
    err, bound = (gb.double() - 2 * terms.sum(dim=(0, 2, 3))).abs(), 64 * 2.0 ** -24 * 2 * terms.abs().sum(dim=(0, 2, 3))
    print("bias sums: error", err.tolist(), "bound", bound.tolist())
    assert bool((err <= bound).all()), (err, bound)

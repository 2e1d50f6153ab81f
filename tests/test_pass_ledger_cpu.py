"""The pass bookkeeping of the engine (engine.PassLedger, engine._Pass) without the library or a GPU: CPU uint8 workspaces, and a toy
autograd.Function that claims its pass exactly as vit_3d._ViTFunction does (record and claim token on ctx when a graph is recorded)."""
import sys

import pytest
import torch

from neurovit_amd.engine import PassLedger, _Pass

B, DEV = 2, "cpu"


def forward(led, layout=1, step=False, **form) -> _Pass:
    """what VitRuntime._forward does around its C call; step: the one-call train step (primary workspace, a done pass)"""
    ws = led.workspace(B, True, DEV) if step else led.acquire(B, layout, DEV)
    return led.open(_Pass(B, layout, ws, None, done=step, **form))


class Toy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, led, x, need_grad):
        ctx.led = led
        rec = forward(led, 1 if need_grad else 0)
        ctx.rec = rec if need_grad else None
        ctx.claim = rec.claim() if need_grad else None
        return x * 2.0

    @staticmethod
    def backward(ctx, dy):
        if ctx.rec is None or not ctx.led.pass_is_live(ctx.rec):
            raise RuntimeError("activations have been overwritten")
        ctx.led.backward_pass(ctx.rec).finish()          # a whole backward of THIS pass
        return None, dy * 2.0, None


def model(led, x):
    return Toy.apply(led, x, torch.is_grad_enabled() and x.requires_grad)


@pytest.fixture
def led():
    return PassLedger(lambda b, layout: 1024 * (1 + layout))


@pytest.fixture
def x():
    return torch.ones(3, requires_grad=True)


def forward_backward_loop(led, x):
    for _ in range(3):
        model(led, x).sum().backward()
    return led.extra_workspaces(B, DEV), led.current.ws is led.workspace(B, True, DEV)


def dropped_forwards(led, x):
    for _ in range(3):
        model(led, x)
    return led.extra_workspaces(B, DEV), led.current.ws is led.workspace(B, True, DEV)


def test_two_forwards_before_one_backward_take_two_workspaces(led, x):
    y1 = model(led, x)
    first = led.current
    y2 = model(led, x)
    assert led.extra_workspaces(B, DEV) == 1
    assert first.ws is led.workspace(B, True, DEV) and led.current.ws is not first.ws
    assert led.pass_is_live(first) and led.pass_is_live(led.current)
    (y1.sum() + y2.sum()).backward()
    assert first.done and led.current.done and led.extra_workspaces(B, DEV) == 1
    assert x.grad.tolist() == [4.0, 4.0, 4.0]


def test_forward_backward_loop_needs_one_workspace(led, x):
    assert forward_backward_loop(led, x) == (0, True)


def test_dropped_forwards_need_one_workspace(led, x):
    assert dropped_forwards(led, x) == (0, True)


@pytest.mark.parametrize("loop", [forward_backward_loop, dropped_forwards])
def test_a_foreign_reference_or_a_tracer_changes_nothing(led, x, loop):
    """what a reference count could not tell apart: someone else holding the current record, and a trace function holding frames"""
    kept = []
    for _ in range(3):
        model(led, x)
        kept.append(led.current)                         # a user, a debugger: further references to the record
    assert led.extra_workspaces(B, DEV) == 0
    assert loop(led, x) == (0, True)
    seen = []
    old = sys.gettrace()
    sys.settrace(lambda frame, event, arg: seen.append(event) and None)
    try:
        got = loop(led, x)
    finally:
        sys.settrace(old)
    assert seen and got == (0, True)


def test_no_grad_claims_nothing(led, x):
    with torch.no_grad():
        model(led, x)
    assert led.last.layout == 0 and led.current is None and not led.last.held


def test_retained_graph_backward_twice_then_stale(led, x):
    y = model(led, x)
    old = led.current
    y.sum().backward(retain_graph=True)
    y.sum().backward(retain_graph=True)                  # twice in a row is fine: nothing has refilled the workspace
    assert old.done and old.held and led.pass_is_live(old)
    y2 = model(led, x)                                   # the old pass has had its backward: its workspace is refilled
    assert led.current.ws is old.ws and not led.pass_is_live(old) and led.extra_workspaces(B, DEV) == 0
    with pytest.raises(RuntimeError, match="activations have been overwritten"):
        y.sum().backward()
    with pytest.raises(RuntimeError, match="activations have been overwritten"):
        led.backward_pass(old)
    y2.sum().backward()


def test_a_train_step_makes_a_pending_pass_in_the_primary_workspace_stale(led, x):
    y = model(led, x)
    pending = led.current
    step = forward(led, step=True)
    assert step.ws is pending.ws and step.done and step.grad_ready and led.last is step and led.current is step
    assert not led.pass_is_live(pending) and led.pass_is_live(step)
    with pytest.raises(RuntimeError, match="activations have been overwritten"):
        y.sum().backward()


@pytest.mark.parametrize("layout", [0, 2])
def test_an_inference_forward_between_a_training_forward_and_its_backward(led, x, layout):
    y = model(led, x)
    pending = led.current
    between = forward(led, layout)
    assert led.last is between and between.layout == layout and led.current is pending and led.pass_is_live(pending)
    assert not led.last.grad_ready
    y.sum().backward()                                   # a backward of an OLDER pass: its own record is ready, the last one's is not
    assert pending.done and pending.grad_ready and not led.last.grad_ready
    y = model(led, x)
    assert not led.last.grad_ready
    y.sum().backward()
    assert led.last.grad_ready and led.last is led.current


def test_a_replayed_step_reinstalls_its_own_record(led, x):
    sigma, inp = object(), object()
    captured = forward(led, step=True, keep=(sigma, inp), rows_form=2, dropout=(0.0, 0.0, 77))
    captured.dlogits = torch.zeros(B, 2)
    forward(led, 1, keep=(None, None), rows_form=1, dropout=(0.1, 0.1, 5))        # a validation forward in the training layout ...
    forward(led, 0, rows_form=1)                                                  # ... and one in the inference layout in between
    assert not led.pass_is_live(captured)
    assert led.note_step_replayed(captured) is captured
    assert led.last is captured and led.current is captured and led.pass_is_live(captured)
    assert captured.keep == (sigma, inp) and captured.rows_form == 2 and captured.dropout == (0.0, 0.0, 77)
    assert captured.done and captured.grad_ready and captured.layout == 1
    assert led.backward_pass() is captured and led.extra_workspaces(B, DEV) == 0


def test_workspaces_are_cached_per_layout_aligned_and_sized(led):
    a, b, c = (led.workspace(B, k, DEV) for k in (0, 1, 2))
    assert [t.numel() for t in (a, b, c)] == [1024, 2048, 3072] and all(t.data_ptr() % 256 == 0 for t in (a, b, c))
    assert led.workspace(B, True, DEV) is b and led.acquire(B, 0, DEV) is a and led.acquire(B, 2, DEV) is c
    assert led.extra_workspaces(B, DEV) == 0 and led.extra_workspaces(B + 1, DEV) == 0

"""Where the optimizer update runs (TrainStep._plan -> UpdatePlan, the table of DESIGN.md "Where the update runs"), without a GPU:
the placement of literal option rows, the refusals, and the whole cross product of the options against the rules restated here."""
import itertools

import pytest
import torch

import weights as W

F = 4096            # TrainStep.FUSE_MAX_ROWS, written out: the rows below are literal


@pytest.fixture(scope="module")
def step():
    """One step on a CPU-resident model whose ViT has phantom slots (heads == 1, dim == dim_head) and whose arena is grouped
    (no_decay: two weight decays); _set switches the options _plan reads."""
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.trainer import TrainStep
    size = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=1, TRAINING_VIT_MLP_DIM=128)
    s = TrainStep(ne.NeuroEncoder(W.neuro_config(32, 8, DEVICE="cpu", **size)), weight_decay=0.05, no_decay=True)
    assert TrainStep.FUSE_MAX_ROWS == F
    s._vit.flat_parameters()
    s._real_phantom = s._vit._phantom
    s._real_decay = [g["weight_decay"] for g in s.optimizer.param_groups]
    assert len(s._real_phantom) > 0 and len(set(s._real_decay)) == 2 and s.optimizer.is_grouped(s._vit)
    return s


def _set(step, acc, scaler, clipper, grouped, phantom, native_dp, fuse, graphs, msg16=True):
    step.accumulation_steps = acc
    step.scaler = object() if scaler else None              # (_plan asks only whether there is one)
    step.clipper = object() if clipper else None
    for g, wd in zip(step.optimizer.param_groups, step._real_decay):      # a scheduler rewriting the groups: _plan re-reads them every step
        g["weight_decay"] = wd if grouped else 0.0
    step._vit._phantom = step._real_phantom if phantom else []
    step._ncomm = object() if native_dp else None
    step.fuse_update = fuse
    step._graphs_on = bool(graphs)
    step._dp_msg16 = msg16


def _got(step, rows, dropout, loss_opts):
    p = step._plan(rows, bool(dropout), bool(loss_opts))
    return (p.whole_gradient, p.fuse, p.behind, p.graph_ok, p.dp_per_bucket, p.dp_msg16)


RAISES = "parameter groups"       # grouped under the native data-parallel plan: ValueError
# accumulation, scaler, clipper, grouped, phantom, native-dp, fuse_update, rows, dropout, loss options, graphs
#     -> whole_gradient, fuse, behind, graph_ok, dp_per_bucket, dp_msg16 (16-bit messages requested)
TABLE = [
    # nothing on: the requested mode, None = by rows
    ((1, 0, 0, 0, 0, 0, None, F,     0, 0, 0), (0, 3, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 0, 0, None, F + 1, 0, 0, 0), (0, 0, 0, 0, 0, 1)),
    ((1, 0, 0, 0, 0, 0, 0,    F,     0, 0, 0), (0, 0, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 0, 0, 1,    F,     0, 0, 0), (0, 1, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 0, 0, 2,    F,     0, 0, 0), (0, 2, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 0, 0, 3,    F,     0, 0, 0), (0, 3, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 0, 0, 0,    F + 1, 0, 0, 0), (0, 0, 0, 0, 0, 1)),
    ((1, 0, 0, 0, 0, 0, 1,    F + 1, 0, 0, 0), (0, 1, 0, 0, 0, 1)),
    ((1, 0, 0, 0, 0, 0, 2,    F + 1, 0, 0, 0), (0, 2, 0, 0, 0, 1)),
    ((1, 0, 0, 0, 0, 0, 3,    F + 1, 0, 0, 0), (0, 3, 0, 0, 0, 1)),
    ((1, 0, 0, 0, 0, 0, None, F,     1, 0, 0), (0, 3, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 0, 0, None, F,     0, 1, 0), (0, 3, 0, 0, 1, 1)),
    # graphs on: what keeps a step away from the replay
    ((1, 0, 0, 0, 0, 0, None, F,     0, 0, 1), (0, 3, 0, 1, 1, 1)),
    ((1, 0, 0, 0, 0, 0, None, F + 1, 0, 0, 1), (0, 0, 0, 1, 0, 1)),
    ((1, 0, 0, 0, 0, 0, 1,    F,     0, 0, 1), (0, 1, 0, 1, 1, 1)),
    ((1, 0, 0, 0, 0, 0, None, F,     1, 0, 1), (0, 3, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 0, 0, None, F,     0, 1, 1), (0, 3, 0, 0, 1, 1)),
    ((2, 0, 0, 0, 0, 0, None, F,     0, 0, 1), (0, 0, 0, 0, 0, 1)),
    ((1, 1, 0, 0, 0, 0, None, F,     0, 0, 1), (1, 0, 0, 0, 0, 0)),
    ((1, 0, 1, 0, 0, 0, None, F,     0, 0, 1), (1, 0, 1, 0, 1, 1)),
    ((1, 0, 0, 1, 0, 0, None, F,     0, 0, 1), (1, 0, 1, 1, 1, 1)),      # a grouped arena stays eligible: the replay ends in the arena launch
    ((1, 0, 0, 1, 0, 0, None, F,     1, 0, 1), (1, 0, 1, 0, 1, 1)),
    ((1, 0, 0, 0, 1, 0, None, F,     0, 0, 1), (0, 0, 0, 1, 1, 1)),
    ((1, 0, 0, 0, 0, 1, None, F,     0, 0, 1), (0, 0, 0, 0, 1, 1)),      # no graph under the native data-parallel plan: it holds no all-reduce
    ((1, 1, 0, 0, 0, 1, None, F,     0, 0, 1), (1, 0, 0, 0, 0, 0)),
    # accumulation
    ((2, 0, 0, 0, 0, 0, None, F,     0, 0, 0), (0, 0, 0, 0, 0, 1)),
    ((2, 0, 0, 0, 0, 0, 1,    F,     0, 0, 0), (0, 0, 0, 0, 0, 1)),
    ((2, 0, 0, 0, 0, 0, 2,    F,     0, 0, 0), (0, 0, 0, 0, 0, 1)),
    ((2, 0, 0, 0, 0, 0, 3,    F,     0, 0, 0), (0, 0, 0, 0, 0, 1)),
    # a scaler: the whole gradient first, but the update stays inside the call
    ((1, 1, 0, 0, 0, 0, 3,    F,     0, 0, 0), (1, 0, 0, 0, 0, 0)),
    ((2, 1, 0, 0, 0, 0, None, F,     0, 0, 0), (1, 0, 0, 0, 0, 0)),
    ((1, 1, 0, 0, 0, 1, 3,    F,     0, 0, 0), (1, 0, 0, 0, 0, 0)),
    ((1, 1, 1, 0, 0, 0, None, F,     0, 0, 0), (1, 0, 1, 0, 0, 0)),
    ((1, 1, 0, 1, 0, 0, None, F,     0, 0, 0), (1, 0, 1, 0, 0, 0)),
    # a clipper, a grouped arena: FusedAdamW.step behind the call
    ((1, 0, 1, 0, 0, 0, 2,    F,     0, 0, 0), (1, 0, 1, 0, 1, 1)),
    ((1, 0, 1, 0, 0, 0, None, F + 1, 0, 0, 0), (1, 0, 1, 0, 0, 1)),
    ((2, 0, 1, 0, 0, 0, None, F,     0, 0, 0), (1, 0, 1, 0, 0, 1)),
    ((1, 0, 1, 1, 0, 0, None, F,     0, 0, 0), (1, 0, 1, 0, 1, 1)),
    ((1, 0, 1, 0, 0, 1, None, F,     0, 0, 0), (1, 0, 1, 0, 1, 1)),      # (the constructor builds no native plan beside a clipper)
    ((1, 0, 0, 1, 0, 0, 3,    F,     0, 0, 0), (1, 0, 1, 0, 1, 1)),
    ((1, 0, 0, 1, 0, 0, 1,    F + 1, 0, 0, 0), (1, 0, 1, 0, 0, 1)),
    ((2, 0, 0, 1, 0, 0, None, F,     1, 1, 0), (1, 0, 1, 0, 0, 1)),
    ((1, 0, 0, 1, 1, 0, None, F,     0, 0, 0), (1, 0, 1, 0, 1, 1)),
    # grouped under the native data-parallel plan: refused, whatever else is set
    ((1, 0, 0, 1, 0, 1, None, F,     0, 0, 0), RAISES),
    ((1, 1, 0, 1, 0, 1, 0,    F,     0, 0, 0), RAISES),
    ((2, 0, 1, 1, 1, 1, 3,    F + 1, 1, 1, 1), RAISES),
    # phantom slots, the native data-parallel plan: fuse 0
    ((1, 0, 0, 0, 1, 0, 3,    F,     0, 0, 0), (0, 0, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 1, 0, 1,    F + 1, 0, 0, 0), (0, 0, 0, 0, 0, 1)),
    ((1, 0, 0, 0, 1, 1, 2,    F,     0, 0, 0), (0, 0, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 0, 1, 3,    F,     0, 0, 0), (0, 0, 0, 0, 1, 1)),
    ((1, 0, 0, 0, 0, 1, None, F + 1, 0, 0, 0), (0, 0, 0, 0, 0, 1)),
    ((2, 0, 0, 0, 0, 1, None, F,     0, 0, 0), (0, 0, 0, 0, 0, 1)),
    ((1, 0, 0, 0, 0, 1, None, F,     1, 1, 0), (0, 0, 0, 0, 1, 1)),
    # everything but the groups at once
    ((2, 1, 1, 0, 1, 1, 3,    F + 1, 1, 1, 1), (1, 0, 1, 0, 0, 0)),
]


@pytest.mark.parametrize("options,want", TABLE, ids=["-".join(map(str, options)) for options, _ in TABLE])
def test_placement_table(step, monkeypatch, options, want):
    monkeypatch.delenv("NEUROVIT_DP_UPDATE_PER_BUCKET", raising=False)
    acc, scaler, clipper, grouped, phantom, native_dp, fuse, rows, dropout, loss_opts, graphs = options
    _set(step, acc, scaler, clipper, grouped, phantom, native_dp, fuse, graphs)
    if want == RAISES:
        with pytest.raises(ValueError, match=RAISES):
            step._plan(rows, bool(dropout), bool(loss_opts))
        return
    assert _got(step, rows, dropout, loss_opts) == want
    step._dp_msg16 = False                                   # fp32 messages requested: never 16-bit ones
    assert _got(step, rows, dropout, loss_opts) == want[:5] + (0,)


def test_per_bucket_override_applies_only_where_the_rule_allows_per_bucket_updates(step, monkeypatch):
    for value in ("0", "1", "2"):
        monkeypatch.setenv("NEUROVIT_DP_UPDATE_PER_BUCKET", value)
        _set(step, 1, 0, 0, 0, 0, 1, None, 0)
        assert _got(step, F, 0, 0)[4] == int(value) and _got(step, F + 1, 0, 0)[4] == 0
        _set(step, 1, 1, 0, 0, 0, 1, None, 0)
        assert _got(step, F, 0, 0)[4] == 0
        _set(step, 2, 0, 0, 0, 0, 1, None, 0)
        assert _got(step, F, 0, 0)[4] == 0


def test_every_combination_follows_the_rules(step, monkeypatch):
    """The whole cross product (5120 option sets x 16-bit messages requested or not) against the rules as DESIGN.md states them,
    restated here independently of the code under test.  None is skipped: what is refused must raise."""
    monkeypatch.delenv("NEUROVIT_DP_UPDATE_PER_BUCKET", raising=False)
    seen = 0
    for acc, scaler, clipper, grouped, phantom, ndp, fuse, graphs, msg16 in itertools.product((1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1),
                                                                                              (None, 0, 1, 2, 3), (0, 1), (0, 1)):
        _set(step, acc, scaler, clipper, grouped, phantom, ndp, fuse, graphs, bool(msg16))
        for rows, dropout, loss_opts in itertools.product((F, F + 1), (0, 1), (0, 1)):
            seen += 1
            if grouped and ndp:
                with pytest.raises(ValueError, match=RAISES):
                    step._plan(rows, bool(dropout), bool(loss_opts))
                continue
            whole = bool(scaler or clipper or grouped)
            want_fuse = (3 if rows <= F else 0) if fuse is None else fuse
            if acc != 1 or phantom or whole or ndp:
                want_fuse = 0
            want = (whole, want_fuse, bool(clipper or grouped),
                    bool(graphs and acc == 1 and not dropout and not scaler and not clipper and not loss_opts and not ndp),
                    int(not scaler and acc == 1 and rows <= F), bool(msg16 and not scaler))
            assert _got(step, rows, dropout, loss_opts) == want, (acc, scaler, clipper, grouped, phantom, ndp, fuse, graphs, msg16, rows, dropout, loss_opts)
    assert seen == 2 * 5120


def test_plan_is_a_frozen_record_and_does_no_tensor_work(step, monkeypatch):
    from dataclasses import FrozenInstanceError
    _set(step, 1, 0, 0, 0, 0, 0, None, 0)
    plan = step._plan(F, False, False)
    with pytest.raises(FrozenInstanceError):
        plan.fuse = 1

    def refuse(*a, **k):
        raise AssertionError("_plan must not create a tensor")
    for name in ("empty", "zeros", "tensor", "zeros_like"):
        monkeypatch.setattr(torch, name, refuse)
    assert step._plan(F, False, False) == plan


def test_the_constructor_refuses_each_conflict():
    """overlap_optimizer with clipping, with parameter groups and with a dynamic loss scale - before any device work, so on a CPU model"""
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.trainer import TrainStep
    size = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=1, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=128)
    model = ne.NeuroEncoder(W.neuro_config(32, 8, DEVICE="cpu", **size))
    with pytest.raises(AssertionError, match="max_grad_norm"):
        TrainStep(model, overlap_optimizer=True, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="overlap_optimizer"):
        TrainStep(model, overlap_optimizer=True, layer_decay=0.5)
    with pytest.raises(AssertionError, match="dynamic loss scale"):
        TrainStep(model, overlap_optimizer=True, loss_scale="dynamic")
    # groups with native_dp: the constructor builds no native plan for them (the bucket pipeline takes over) ...
    grouped = TrainStep(model, no_decay=True, native_dp=True)
    assert grouped._ncomm is None and grouped.optimizer.is_grouped()
    # ... and a plan that finds both - groups that a scheduler made distinct later - raises (test_placement_table)

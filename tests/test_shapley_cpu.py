"""CPU checks of Shapley value sampling (no GPU): the restatements of tests/shapley_ref.py that the GPU tests (tests/test_shapley_gpu.py)
compare the kernels with, held to properties that do not depend on them:

  draw         every rank row is a permutation, the antithetic row is the reverse, other seed / unit / sample give other permutations, the keys
               are not nv_mim_labels' keys at the same seed, and with F = 3 all six orders appear over 6000 units, each within 5 sigma of 1000;
  accumulator  a random fp32 game with F = 4 through all 24 permutations gives the exact Shapley values (rational arithmetic) within the
               derived bound and delta within its bound; a dummy player gets exactly 0 with standard error exactly 0; two symmetric players
               get equal values; U = 1 gives a NaN standard error; the standard error is the two-pass one over UNITS;
  defects      a rank off by one, the ends swapped, an antithetic row that is not the reverse, a mean over permutations instead of units:
               each fails the checks above;
  the rest     labels, the rows form of mask_ref, token maps, atlas_to_patch_features' rules, the new entry points and their argument checks,
               the refusals of shapley_values that need no device.
"""
import ctypes

import numpy as np
import pytest
import torch

import mim_ref
import shapley_ref as SR
import weights as W
from test_perturbation_cpu import MICRO_SIZE, mask_ref

SEED = 20


def is_permutation(rows):
    F = rows.shape[-1]
    return bool((torch.sort(rows.long(), dim=-1).values == torch.arange(F)).all())


# ---------------------------------------------------------------------------------------------------------------- the draw

def check_draw(draw):
    """what any draw must satisfy; raises AssertionError"""
    for F in (2, 3, 8, 27):
        both = draw(SEED, 0, 4, 2, 3, F)
        assert both.shape == (8, 3, F) and both.dtype == torch.int32
        assert is_permutation(both)
        assert torch.equal(both[1::2], F - 1 - both[0::2])                      # the antithetic row is the reverse
        assert torch.equal(draw(SEED, 0, 4, 1, 3, F), both[0::2])               # R = 1 draws the same units
        assert torch.equal(draw(SEED, 2, 2, 2, 3, F), both[4:])                 # first_unit shifts the units
    wide = draw(SEED, 0, 6, 1, 4, 27)
    rows = wide.reshape(24, 27)
    assert len({tuple(r.tolist()) for r in rows}) == 24                         # other unit, other sample: other permutations
    assert not torch.equal(draw(SEED + 1, 0, 6, 1, 4, 27), wide)


def test_draw_rows_are_permutations_and_the_antithetic_row_is_the_reverse():
    check_draw(SR.draw_ref)


def test_draw_has_a_domain_of_its_own():
    for unit in (0, 3):
        for b in (0, 2):
            assert SR.player_keys(SEED, unit, b, 64) != mim_ref.unit_keys(SEED, 0, unit, b, 64)
    assert SR.player_keys(SEED, 1, 0, 8) != SR.player_keys(SEED, 0, 1, 8)       # unit and sample are different coordinates


def test_all_six_orders_of_three_players_appear_equally_often():
    U = 6000
    counts = {}
    for u in range(U):
        keys = SR.player_keys(SEED, u, 0, 3)
        order = tuple(sorted(range(3), key=lambda f: (-keys[f], f)))
        counts[order] = counts.get(order, 0) + 1
    sigma = (U * (1 / 6) * (5 / 6)) ** 0.5
    assert len(counts) == 6
    assert all(abs(c - U / 6) <= 5 * sigma for c in counts.values()), counts
    first = SR.draw_ref(SEED, 0, 8, 1, 1, 3)[:, 0]                              # the same orders through draw_ref: rank -> order
    for u in range(8):
        keys = SR.player_keys(SEED, u, 0, 3)
        order = sorted(range(3), key=lambda f: (-keys[f], f))
        assert [int(first[u, f]) for f in order] == [0, 1, 2]


# ---------------------------------------------------------------------------------------------------------------- the accumulator

def antithetic_rows(F):
    """all F! permutations as F! / 2 units of (permutation, reverse): int32 [F!, F]"""
    rows, seen = [], set()
    for r in SR.all_rank_rows(F).tolist():
        if tuple(r) not in seen:
            rev = [F - 1 - v for v in r]
            seen.update((tuple(r), tuple(rev)))
            rows += [r, rev]
    return torch.tensor(rows, dtype=torch.int32)


def check_accumulator(accumulate, antithetic=antithetic_rows):
    """a random fp32 game with F = 4 through all 24 permutations, as 12 antithetic units and as 24 units; raises AssertionError"""
    F = 4
    g = torch.Generator().manual_seed(41)
    game = (torch.randn(1 << F, generator=g) * 3).float()
    M = float(game.abs().max())
    exact = SR.exact_shapley(game.numpy())
    for R, ranks in ((2, antithetic(F)), (1, SR.all_rank_rows(F))):
        interior, ends = SR.game_scores(game, ranks)
        values, stderr, delta, sums = accumulate(interior, ends, ranks.view(-1, 1, F), R)
        U = ranks.shape[0] // R
        assert np.abs(values[0].astype(np.float64) - exact).max() <= SR.value_bound(M, U) + SR.U64 * 2 * M
        assert abs(float(delta[0])) <= SR.delta_bound(M, F, U)
        assert abs(values[0].astype(np.float64).sum() - (float(game[-1]) - float(game[0]))) <= SR.delta_bound(M, F, U) + F * 2.0 ** -24 * M
        # the standard error over UNITS, two-pass in float64; the one-pass variance carries (U + 3) u sumsq / (U - 1), 8 U u sumsq / (U - 1) taken
        marg = np.stack([[float(game[sum(1 << j for j in range(F) if int(r[j]) <= int(r[f]))]) -
                          float(game[sum(1 << j for j in range(F) if int(r[j]) < int(r[f]))]) for f in range(F)] for r in ranks.tolist()])
        unit = marg.reshape(U, R, F).mean(axis=1)
        var = unit.var(axis=0, ddof=1)
        got_var = stderr[0].astype(np.float64) ** 2 * U
        tol = 8 * U * SR.U64 * sums[0, :, 1] / (U - 1) + 2.0 ** -22 * var
        assert (np.abs(got_var - var) <= tol).all(), (R, got_var, var)


def test_accumulator_gives_the_exact_shapley_values_of_a_game():
    check_accumulator(SR.accumulate_ref)


def test_dummy_and_symmetric_players_and_one_unit():
    F = 4
    g = torch.Generator().manual_seed(42)
    base = torch.randint(-50, 50, (1 << (F - 1),), generator=g).float() * 0.37
    # player 3 is a dummy: v[S + 3] = v[S]
    game = torch.cat([base, base])
    ranks = antithetic_rows(F)
    values, stderr, delta, _ = SR.accumulate_ref(*SR.game_scores(game, ranks), ranks.view(-1, 1, F), 2)
    assert values[0, 3] == 0.0 and stderr[0, 3] == 0.0
    assert np.abs(values[0, :3]).min() > 0
    # players 0 and 1 are symmetric: v depends on them through their count; integer values, so every sum is exact
    table = torch.randint(-9, 9, (3, 1 << (F - 2)), generator=g).float()
    sym = torch.tensor([float(table[(m & 1) + (m >> 1 & 1), m >> 2]) for m in range(1 << F)])
    values, _, delta, _ = SR.accumulate_ref(*SR.game_scores(sym, SR.all_rank_rows(F)), SR.all_rank_rows(F).view(-1, 1, F), 1)
    assert values[0, 0] == values[0, 1] and float(delta[0]) == 0.0
    assert np.array_equal(values[0].astype(np.float64), SR.exact_shapley(sym.numpy()).astype(np.float32).astype(np.float64))
    one = SR.all_rank_rows(F)[5:6]
    _, stderr, _, _ = SR.accumulate_ref(*SR.game_scores(sym, one), one.view(1, 1, F), 1)
    assert np.isnan(stderr).all()


def test_planted_defects_fail():
    def off_by_one(interior, ends, ranks, R):
        return SR.accumulate_ref(interior, ends, (ranks + 1) % ranks.shape[-1], R)

    def ends_swapped(interior, ends, ranks, R):
        return SR.accumulate_ref(interior, ends.flip(1), ranks, R)

    def mean_over_permutations(interior, ends, ranks, R):
        return SR.accumulate_ref(interior, ends, ranks, 1)                     # every permutation a unit of its own

    def pairs_not_reversed(F):
        rows = antithetic_rows(F)
        rows[1::2] = rows[0::2]
        return rows
    for broken in (off_by_one, ends_swapped, mean_over_permutations):
        with pytest.raises(AssertionError):
            check_accumulator(broken)
    with pytest.raises(AssertionError):
        check_accumulator(SR.accumulate_ref, antithetic=pairs_not_reversed)    # half the permutations twice: not the Shapley values

    def draw_not_reversed(seed, first_unit, U, R, B, F):
        out = SR.draw_ref(seed, first_unit, U, R, B, F)
        if R == 2:
            out[1::2] = out[0::2]
        return out
    with pytest.raises(AssertionError):
        check_draw(draw_not_reversed)


# ---------------------------------------------------------------------------------------------------------------- labels, copies, maps

def test_labels_rows_and_token_maps():
    g = torch.Generator().manual_seed(43)
    B, N, F, Q = 2, 27, 5, 3
    features = torch.randint(-1, F, (B, N), generator=g).to(torch.int32)
    features[0, 3] = F + 2                                                     # outside [0, F): no player
    ranks = torch.stack([torch.stack([torch.randperm(F, generator=g) for _ in range(B)]) for _ in range(Q)]).to(torch.int32)
    labels = SR.labels_ref(ranks, features)
    assert labels.shape == (Q * B, N)
    for q in range(Q):
        for b in range(B):
            for t in range(N):
                f = int(features[b, t])
                assert int(labels[q * B + b, t]) == (int(ranks[q, b, f]) if 0 <= f < F else F)
    # the rows form of mask_ref: with row == b it is mask_ref
    size, patch = (27,) * 3, (9,) * 3
    x = torch.randn((B,) + size, generator=g)
    jobs3 = torch.tensor([(0, 0, 2), (1, 1, 4), (1, 3, 3), (2, 0, 5)], dtype=torch.int32)
    jobs4 = torch.stack([jobs3[:, 0], jobs3[:, 0], jobs3[:, 1], jobs3[:, 2]], 1)
    sentinel = torch.full((4,) + size, -7.5)
    per_volume = torch.randn((B,) + size, generator=g)
    for baseline in (0.0, per_volume, per_volume[:1]):
        want = mask_ref(x, labels[:B], jobs3, patch, baseline, out=sentinel)
        assert torch.equal(SR.mask_rows_ref(x, labels[:B], jobs4, patch, baseline, out=sentinel).view(torch.int32), want.view(torch.int32))
    other = SR.mask_rows_ref(x, labels, torch.tensor([(0, 4, 1, F), (0, 99, 0, F), (0, -1, 0, F)], dtype=torch.int32), patch, out=sentinel[:3])
    assert torch.equal(other[0], mask_ref(x[:1], labels[4:5], torch.tensor([[0, 1, F]]), patch)[0])
    assert torch.equal(other[1:], sentinel[1:3])
    # token maps: a player's value spread over its patches; no player: 0; per volume the map sums to the values of the players present
    values = torch.randn(B, F, generator=g)
    maps = SR.token_maps_ref(values, features)
    for b in range(B):
        for f in range(F):
            cells = features[b] == f
            if int(cells.sum()):
                assert torch.equal(maps[b][cells], (values[b, f] / cells.sum().float()).expand(int(cells.sum())))
        assert float(maps[b][(features[b] < 0) | (features[b] >= F)].abs().max()) == 0.0


def test_atlas_to_patch_features():
    from neurovit_amd.NeuroEncoder import atlas_to_patch_features, window_block_labels
    S, p = 8, 4
    atlas = torch.zeros(S, S, S, dtype=torch.int64)
    atlas[:4] = 7                                  # i0 < 4
    atlas[4:, :4] = 3                              # i0 >= 4, i1 < 4
    atlas[4:, 4:, 4:] = 12                         # i0 >= 4, i1 >= 4, i2 >= 4; (i0 >= 4, i1 >= 4, i2 < 4) stays background
    features, labels = atlas_to_patch_features(atlas, p)
    assert features.dtype == torch.int32 and labels.tolist() == [3, 7, 12]
    # token t = c2 4 + c0 2 + c1
    assert features.tolist() == [1, 1, 0, -1, 1, 1, 0, 2]
    # majority, ties to the lower label: patch 0 half 7 and half 5 -> 5; then 33 of 64 voxels 7 -> 7
    tie = atlas.clone()
    tie[:4, :4, :2] = 5
    features, labels = atlas_to_patch_features(tie, p)
    assert labels.tolist() == [3, 5, 7, 12] and features.tolist() == [1, 2, 0, -1, 2, 2, 0, 3]
    tie[0, 0, 1] = 7
    features, labels = atlas_to_patch_features(tie, p)
    assert labels.tolist() == [3, 7, 12] and features.tolist() == [1, 1, 0, -1, 1, 1, 0, 2]
    # another background; a patch that is mostly background is no player whatever else it holds
    features, labels = atlas_to_patch_features(atlas, p, background=7)
    assert labels.tolist() == [0, 3, 12] and features.tolist() == [-1, -1, 1, 0, -1, -1, 1, 2]
    for wrong in (atlas.float(), atlas[0], atlas[:, :, :6]):
        with pytest.raises(ValueError, match="atlas"):
            atlas_to_patch_features(wrong, p)
    assert window_block_labels(3, 2).tolist() == [0, 0, 1, 0, 0, 1, 2, 2, 3, 0, 0, 1, 0, 0, 1, 2, 2, 3, 4, 4, 5, 4, 4, 5, 6, 6, 7]
    assert torch.equal(window_block_labels(4, 1), torch.arange(64))


# ---------------------------------------------------------------------------------------------------------------- the C-ABI, the refusals

NAMES = ("nv_mask_patches_rows", "nv_shapley_ranks", "nv_shapley_labels", "nv_shapley_accumulate", "nv_shapley_token_maps")


def test_header_declares_and_library_exports_the_new_entry_points():
    from neurovit_amd import _cabi
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NAMES:
        assert name in _cabi.lib.protos, name
        assert getattr(dll, name) is not None, name
    assert _cabi.ABI_VERSION == 8 and _cabi.lib.nv_abi_version() == 8          # new symbols only: the revision stays
    assert _cabi.lib.protos["nv_shapley_ranks"][1][:2] == [ctypes.c_ulong, ctypes.c_ulong]
    assert _cabi.lib.protos["nv_mask_patches_rows"][1][5] is ctypes.c_int and _cabi.lib.protos["nv_mask_patches_rows"][1][8] is ctypes.c_float


def test_entry_points_check_their_arguments_without_a_gpu():
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import lib

    def i3(*v):
        arr = (ctypes.c_int * 3)(*v)
        return arr, ctypes.cast(arr, ctypes.c_void_p)
    fake = 4096                                            # a non-null, 16-byte aligned address nothing dereferences: the checks come first
    _a, s32 = i3(32, 32, 32)
    _b, p8 = i3(8, 8, 8)
    _c, p5 = i3(8, 5, 8)
    assert lib.nv_mask_patches_rows(fake, 1, s32, p8, fake, 0, fake, 1, 0.0, None, 0, fake, None) == -1 and "Rows" in _cabi.last_error()
    assert lib.nv_mask_patches_rows(fake, 1, s32, p5, fake, 2, fake, 1, 0.0, None, 0, fake, None) == -1 and "whole number" in _cabi.last_error()
    assert lib.nv_mask_patches_rows(fake, 1, s32, p8, fake, 2, fake, 1, 0.0, None, 0, fake + 4, None) == -1 and "16-byte" in _cabi.last_error()
    assert lib.nv_mask_patches_rows(fake, 1, s32, p8, None, 2, fake, 1, 0.0, None, 0, fake, None) == -1
    assert lib.nv_shapley_ranks(0, 0, 1, 1, 1, 8, None, None) == -1
    assert lib.nv_shapley_ranks(0, 0, 1, 3, 1, 8, fake, None) == -1 and "R = 3" in _cabi.last_error()
    assert lib.nv_shapley_ranks(0, 0, 1, 1, 1, 1, fake, None) == -1 and "players" in _cabi.last_error()
    assert lib.nv_shapley_ranks(0, 0, 1, 1, 1, 4097, fake, None) == -1 and "4096" in _cabi.last_error()
    assert lib.nv_shapley_ranks(0, 2 ** 32 - 1, 2, 1, 1, 8, fake, None) == -1 and "2^32" in _cabi.last_error()
    assert lib.nv_shapley_ranks(0, 0, 0, 1, 1, 8, fake, None) == -1
    assert lib.nv_shapley_labels(fake, None, 2, 1, 8, 8, fake, None) == -1
    assert lib.nv_shapley_labels(fake, fake, 0, 1, 8, 8, fake, None) == -1
    assert lib.nv_shapley_accumulate(fake, fake, fake, 1, 1, 1, 1, fake, fake, fake, fake, None) == -1 and "players" in _cabi.last_error()
    assert lib.nv_shapley_accumulate(fake, fake, fake, 1, 0, 1, 4, fake, fake, fake, fake, None) == -1 and "R = 0" in _cabi.last_error()
    assert lib.nv_shapley_accumulate(fake, fake, fake, 1, 1, 1, 4, fake, fake, fake, fake + 4, None) == -1 and "8-byte" in _cabi.last_error()
    assert lib.nv_shapley_accumulate(fake, fake, fake, 0, 1, 1, 4, fake, fake, fake, fake, None) == -1
    assert lib.nv_shapley_token_maps(fake, fake, 1, 4097, 8, fake, None) == -1 and "4096" in _cabi.last_error()
    assert lib.nv_shapley_token_maps(fake, None, 1, 8, 8, fake, None) == -1


def test_argument_errors_without_a_device(tmp_path):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    S = 16
    model = NeuroEncoder(W.neuro_config(S, 8, **MICRO_SIZE))
    x, N = torch.zeros(2, S, S, S), 8
    with pytest.raises(ValueError, match="even"):
        model.shapley_values(x, permutations=5)
    for permutations in (0, -2, 2.5):
        with pytest.raises(ValueError, match="permutations"):
            model.shapley_values(x, permutations=permutations, antithetic=False)
    with pytest.raises(ValueError, match="score"):
        model.shapley_values(x, score="margin")
    with pytest.raises(ValueError, match="window"):
        model.shapley_values(x, window=0)
    with pytest.raises(ValueError, match="players"):
        model.shapley_values(x, window=2)                                       # one block: F = 1
    with pytest.raises(ValueError, match="players"):
        model.shapley_values(x, features=torch.zeros(N, dtype=torch.int32))    # F = 1
    with pytest.raises(ValueError, match="players"):
        model.shapley_values(x, features=torch.full((N,), -1))                 # F = 0
    for wrong in (torch.zeros(N + 1, dtype=torch.int32), torch.zeros(3, N, dtype=torch.int32), torch.zeros(N)):
        with pytest.raises(ValueError, match="features"):
            model.shapley_values(x, features=wrong)
    three = torch.tensor([0, 1, 2, -1, 0, 1, 2, 2])
    rows = torch.tensor([[0, 1, 2], [2, 1, 0]])
    with pytest.raises(ValueError, match="features name player 2"):
        model.shapley_values(x, features=three, ranks=rows[:, :2])
    for wrong in (torch.zeros(3, dtype=torch.int64), rows.float(), rows[:, None, :].expand(2, 3, 3), [[0, 1, 2]]):
        with pytest.raises(ValueError, match="ranks must be"):
            model.shapley_values(x, features=three, ranks=wrong)
    with pytest.raises(ValueError, match="ranks has 3 players"):
        model.shapley_values(x, window=1, ranks=rows)
    with pytest.raises(ValueError, match="permutation_offset"):
        model.shapley_values(x, window=1, permutation_offset=-1)
    with pytest.raises(ValueError, match="permutation_offset.*label cells|label cells.*permutation_offset"):
        model.shapley_values(x, window=1, permutations=2 ** 23)
    with pytest.raises(ValueError, match="x must be"):
        model.shapley_values(torch.zeros(2, S, S, 8))
    with pytest.raises(ValueError, match="method"):
        model.attribution_volumes(x, method="lime")
    torch.save(model.state_dict(), tmp_path / "c.pth")
    four_d = NeuroEncoder(W.neuro_config(S, 8, dim=4, GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth", **MICRO_SIZE))
    with pytest.raises(NotImplementedError, match="3D model only"):
        four_d.shapley_values(x)

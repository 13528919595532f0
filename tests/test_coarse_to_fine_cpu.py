"""CPU: the merge-rank rule of coarse_to_fine_kernel (csrc/raypath.hip) stated in numpy and held against
torch.sort(stable=True) of cat(coarse, fine).

The rule: with both runs non-decreasing, coarse element i lands at i + #(fine < coarse[i]) and fine element j at
j + #(coarse <= fine[j]).  The kernel takes it only for rays whose runs pass the neighbour compare `a[e] <= a[e+1]` (which a
NaN fails); every other ray keeps the counting sort."""
import numpy as np
import torch


def merge_ranks(coarse, fine):
    coarse, fine = np.asarray(coarse, np.float32), np.asarray(fine, np.float32)
    rank_c = np.arange(len(coarse)) + np.searchsorted(fine, coarse, side="left")    # #(fine < v)
    rank_f = np.arange(len(fine)) + np.searchsorted(coarse, fine, side="right")     # #(coarse <= v)
    return np.concatenate([rank_c, rank_f])


def stable_ranks(coarse, fine):
    both = torch.cat([torch.as_tensor(np.asarray(coarse, np.float32)), torch.as_tensor(np.asarray(fine, np.float32))])
    order = torch.sort(both, stable=True).indices.numpy()       # order[p] = the element at sorted position p
    ranks = np.empty(len(order), np.int64)
    ranks[order] = np.arange(len(order))
    return ranks


def runs_sorted(coarse, fine):
    ok = lambda a: bool(np.all(np.asarray(a, np.float32)[:-1] <= np.asarray(a, np.float32)[1:]))
    return ok(coarse) and ok(fine)


CASES = {
    "interleaved": ([0.0, 0.2, 0.4, 0.6], [0.1, 0.3, 0.5]),
    "ties_inside_coarse": ([0.0, 0.25, 0.25, 0.25, 1.0], [0.1, 0.5]),
    "ties_inside_fine": ([0.0, 0.5, 1.0], [0.3, 0.3, 0.3, 0.7, 0.7]),
    "ties_across_runs": ([0.0, 0.5, 1.0], [0.0, 0.5, 0.5, 1.0]),
    "ties_inside_and_across": ([0.5, 0.5, 0.5], [0.5, 0.5]),
    "signed_zeros_tie": ([-0.0, 0.0, 1.0], [0.0, -0.0]),
    "all_fine_below": ([2.0, 3.0, 4.0], [0.0, 1.0]),            # #(coarse <= v) = 0 for every fine element
    "all_fine_above": ([0.0, 1.0, 2.0], [3.0, 4.0]),            # #(fine < v) = 0 for every coarse element
    "all_fine_below_touching": ([1.0, 2.0, 3.0], [1.0, 1.0]),   # a tie at the lower end: coarse first
    "all_fine_above_touching": ([1.0, 2.0, 3.0], [3.0, 3.0]),
    "one_fine": ([0.0, 0.5, 1.0], [0.5]),
}


def test_merge_rank_rule_is_the_stable_sort():
    for name, (coarse, fine) in CASES.items():
        assert runs_sorted(coarse, fine), name
        got, want = merge_ranks(coarse, fine), stable_ranks(coarse, fine)
        assert np.array_equal(got, want), (name, got, want)
        assert sorted(got) == list(range(len(coarse) + len(fine))), name      # a permutation: every slot written once


def test_merge_rank_rule_random_runs_with_ties():
    rng = np.random.default_rng(0)
    for n, nf in ((3, 1), (16, 16), (64, 64), (67, 5), (128, 64), (256, 256)):
        for levels in (4, 32, 100000):    # few levels: many ties inside and across the runs
            coarse = np.sort(rng.integers(0, levels, n)).astype(np.float32) / levels
            fine = np.sort(rng.integers(0, levels, nf)).astype(np.float32) / levels
            assert np.array_equal(merge_ranks(coarse, fine), stable_ranks(coarse, fine)), (n, nf, levels)


def test_rule_needs_sorted_runs_and_the_check_sees_it():
    """What the wave's neighbour compares must reject: a descending run, a single inversion, a NaN."""
    desc = ([1.0, 0.5, 0.0], [0.2, 0.4])
    assert not runs_sorted(*desc)
    assert not np.array_equal(merge_ranks(*desc), stable_ranks(*desc))
    assert not runs_sorted([0.0, 0.5, 1.0], [0.4, 0.3999999])
    assert not runs_sorted([0.0, np.nan, 1.0], [0.5])
    assert not runs_sorted([0.0, 0.5, 1.0], [0.5, np.nan])
    assert not runs_sorted([0.0, 0.5, 1.0], [np.nan, 0.5])

"""Grouped allow-lists (rpt_*_allow_group_*) without a GPU: the bitmaps' layout, the restatement
tests/allow_group_ref.py on the standing case of tests/test_gpu_allow_group.py (so that the GPU test
cannot pass by ignoring `group`, by using row 0 for everyone or by striding the rows by n / 32), and
the names through the header, the Python package and the Haskell binding."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allow_group_ref as gref  # noqa: E402
import graph_search_allow_ref as aref  # noqa: E402
import graph_search_ref as sref  # noqa: E402
import test_gpu_graph_search_allow as gsa  # noqa: E402  (helpers only: the lattice, the graph, the seeds)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rpt_graph_search_allow_group_host", "rpt_graph_search_allow_group_dev", "rpt_knn_allow_group_host",
                "rpt_knn_allow_group_dev", "rpt_allow_group_candidates_host", "rpt_brute_knn_allow_group_host",
                "rpt_brute_knn_allow_group_dev", "rpt_recall_hits_allow_group_host")
N, NQ = 500, 64


# ------------------------------------------------------------------ allowBitmaps
def test_allow_bitmaps_rows_are_ceil_n_over_32_words():
    import rptree_amd as rp
    masks = gref.standing_masks(N)
    words = rp.allowBitmaps(masks, N)
    assert words.dtype == np.uint32 and words.shape == (7, 16) and words.flags["C_CONTIGUOUS"]
    assert words.strides[0] == 16 * 4 and 16 != N // 32             # the row stride is ceil(n / 32), not n / 32
    for g, m in enumerate(masks):
        assert np.array_equal(aref.mask_of(words[g], N), m), g
        assert int(words[g, -1]) >> (N % 32) == 0, g                # the bits behind n are clear
        assert np.array_equal(words[g], aref.words_of(m)), g
    assert words[3, -1] == (1 << (N % 32)) - 1 and not words[4].any()
    assert words[5, (N - 2) >> 5] == 1 << ((N - 2) & 31) and np.count_nonzero(words[5]) == 1


def test_allow_bitmaps_takes_masks_ids_and_words():
    import rptree_amd as rp
    masks = gref.standing_masks(N)
    want = rp.allowBitmaps(masks, N)
    mixed = [masks[0], np.flatnonzero(masks[1]), want[2], masks[3], np.zeros(0, dtype=np.int64), [N - 2],
             np.flatnonzero(masks[6]).astype(np.int32)]
    assert np.array_equal(rp.allowBitmaps(mixed, N), want)
    assert np.array_equal(rp.allowBitmaps(np.array(masks), N), want)        # bool[G][n]
    assert rp.allowBitmaps(want, N) is want or np.array_equal(rp.allowBitmaps(want, N), want)
    assert rp.allowBitmaps([], N).shape == (0, 16)
    for bad in ([masks[0][:-1]], [np.array([0, N])], [np.array([-1])], [want[0][:-1]], want[:, :-1],
                [np.array([0.5, 1.5])]):
        with pytest.raises(ValueError):
            rp.allowBitmaps(bad, N)


# ------------------------------------------------------------------ the standing case is not vacuous
def standing_case():
    X = gsa.lattice_rows(24, N, 24)
    Q = gsa.lattice_queries(X, np.random.default_rng(100 + 24), NQ)
    gids, gcnt = gsa.make_graph(np.random.default_rng(10), N, 10)
    seeds = gsa.make_seeds(np.random.default_rng(66), NQ, N, 8)
    return X, Q, gids, gcnt, seeds, gref.standing_masks(N), gref.standing_group(NQ)


def test_the_standing_group_interleaves():
    group = gref.standing_group(NQ)
    assert sorted(np.unique(group).tolist()) == list(range(-1, 7))
    assert all((group == g).sum() == 8 for g in range(-1, 7))
    blocks = [len(set(group[b:b + 4].tolist())) for b in range(0, NQ, 4)]
    assert len(blocks) == 16 and min(blocks) >= 3, blocks               # a workgroup of four waves mixes groups


@pytest.mark.parametrize("metric", gsa.METRICS)
def test_the_standing_case_tells_the_bitmaps_apart(metric):
    X, Q, gids, gcnt, seeds, masks, group = standing_case()
    D = sref.query_matrix(X, Q, metric)
    k = 10
    for ef, width in ((32, 32), (32, 128), (16, 1024)):
        (wi, wd, wc), exp, offered, upper = gref.group_answers(X, Q, gids, gcnt, seeds, k, ef, width, masks, group,
                                                               metric, D=D)
        # the composition is the single-bitmap restatement, query by query
        for q in (0, 1, 2, 3, 17, 63):
            one, e1, _, _ = aref.graph_search_allow_ref(X, Q[q:q + 1], gids, gcnt, seeds[q:q + 1], k, ef, width,
                                                        gref.mask_of_group(masks, int(group[q]), N), metric,
                                                        D=D[q:q + 1])
            sref.assert_same_answer((wi[q:q + 1], wd[q:q + 1], wc[q:q + 1]), one, "query %d" % q)
        assert offered <= upper and exp > 0
        row0, _, _, _ = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, k, ef, width, masks[0], metric, D=D)
        plain, _, _, _ = aref.graph_search_allow_ref(X, Q, gids, gcnt, seeds, k, ef, width, None, metric, D=D)
        not0 = np.flatnonzero(group != 0)
        filtered = np.flatnonzero(group != -1)
        other_than_row0 = sum(not np.array_equal(wi[q], row0[0][q]) for q in not0)
        other_than_plain = sum(not np.array_equal(wi[q], plain[0][q]) for q in filtered)
        print("%s ef %d width %d: %d of %d differ from bitmap 0, %d of %d from the unfiltered answer" %
              (metric, ef, width, other_than_row0, len(not0), other_than_plain, len(filtered)))
        assert len(not0) == 56 and 4 * other_than_row0 >= 3 * len(not0)
        assert len(filtered) == 56 and 4 * other_than_plain >= 3 * len(filtered)
        # a row stride of n / 32 = 15 words instead of 16 reads other masks for every row but the first
        words = gref.words_of_masks(masks, N)
        flat = words.reshape(-1)
        shifted = [aref.mask_of(flat[g * (N // 32):g * (N // 32) + 16], N) for g in range(7)]
        assert all(not np.array_equal(shifted[g], masks[g]) for g in (1, 2, 3, 5, 6))
        # what the all-zeros group, the single id and the unfiltered group must answer
        assert np.all(wc[group == 4] == 0)
        assert np.all(wc[group == 5] <= 1) and np.all(wi[group == 5][:, 0][wc[group == 5] == 1] == N - 2)
        assert np.array_equal(wi[group == -1], plain[0][group == -1])


# ------------------------------------------------------------------ the names, through every layer
def test_the_header_declares_the_eight_entry_points():
    text = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        decl = re.findall(r"int32_t %s\(([^;]*)\);" % name, code)
        assert len(decl) == 1, name
        allow, group = ("allow_host", "group_host") if name.endswith("_host") else ("allow_dev", "group_dev")
        args = [a.strip() for a in decl[0].split(",")]
        at = [i for i, a in enumerate(args) if a.endswith(" " + allow)]
        assert len(at) == 1, name
        assert args[at[0]] == "const uint32_t* " + allow and args[at[0] + 1] == "int32_t G" and \
            args[at[0] + 2] == "const int32_t* " + group, (name, args[at[0]:at[0] + 3])
        # the rest of the list is the single-bitmap entry point's
        single = re.findall(r"int32_t %s\(([^;]*)\);" % name.replace("_allow_group_", "_allow_"), code)
        assert len(single) == 1, name
        rest = [a.strip() for a in single[0].split(",")]
        assert args[:at[0] + 1] + args[at[0] + 3:] == rest, name
    assert "knn_allow_group_budget" in text


def test_the_python_package_exports_the_new_names():
    import rptree_amd as rp
    from rptree_amd import _lib
    for name in ("allowBitmaps", "graphSearchAllowGroup", "graphSearchAllowGroupDev", "knnAllowGroup",
                 "knnAllowGroupDev", "allowGroupCandidates", "bruteKnnAllowGroup", "bruteKnnAllowGroupDev",
                 "recallHitsAllowGroup", "recallWithAllowGroupBatch"):
        assert name in rp.__all__ and callable(getattr(rp, name)), name
    for name in ENTRY_POINTS:
        assert name in _lib.SYMBOLS, name
        single = _lib.SYMBOLS[name.replace("_allow_group_", "_allow_")][1]
        args = _lib.SYMBOLS[name][1]
        assert len(args) == len(single) + 2, name
    # The single-bitmap functions keep the signatures the existing tests pin; the grouped form of each
    # is a function of its own that takes `group` behind `allow`, the rest of the list unchanged.
    import inspect
    params = lambda fn: list(inspect.signature(getattr(rp, fn)).parameters)  # noqa: E731
    for single, grouped in (("graphSearchAllow", "graphSearchAllowGroup"), ("knnAllow", "knnAllowGroup"),
                            ("allowCandidates", "allowGroupCandidates"), ("bruteKnnAllow", "bruteKnnAllowGroup"),
                            ("recallHitsAllow", "recallHitsAllowGroup"),
                            ("recallWithAllowBatch", "recallWithAllowGroupBatch")):
        assert params(grouped) == ["allow", "group"] + params(single)[1:], grouped


def test_the_haskell_binding_names_them():
    text = open(os.path.join(ROOT, "haskell", "Data", "RPTree", "HIP.hs")).read()
    for name in ENTRY_POINTS:
        assert re.search(r'foreign import ccall (safe|unsafe)? *"%s"' % name, text), name

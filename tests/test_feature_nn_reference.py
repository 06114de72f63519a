"""CPU: the float64 comparison of tests/test_gpu_feature_nn.py is pinned before a kernel is called.  Every case admitted to
it must let a float32 restatement (torch float32 of the reference's expression, reduced with "minimum, then lowest index")
pass the same comparison, with at most 2 % of its rows and of its columns unclear; the comparison itself must refuse planted
errors; and the helpers must agree with the reference's own index logic."""
import numpy as np
import pytest

import feature_nn_cases as C
import feature_nn_f64 as F64

NORMALIZED_F64 = ("1300x1200x36_unit", "65x63x33_gauss", "2000x1500x32_gauss")   # as tests/test_gpu_feature_nn.py


def test_strip_rule_and_case_table():
    assert C.strip_tiles(8192, 8192) == 8 and C.strip_tiles(25000, 25000) == 10 and C.strip_tiles(200_000, 200_000) == 521
    assert C.strip_tiles(1, 1) == 1 and C.strip_tiles(1700, 1700) == 1 and C.strip_tiles(*C.STRIP_SHAPE[:2]) == 2
    assert not C.BY_NAME["1665x1700x3_room"].f64 and "1665x1700x3_room" not in C.F64_CASES
    for case in C.CASES:
        x, y = C.build(case.name)
        assert x.dtype == y.dtype == np.float32 and x.shape == (case.n, case.c) and y.shape == (case.m, case.c)


@pytest.mark.parametrize("name,normalized", [(n, False) for n in C.F64_CASES] + [(n, True) for n in NORMALIZED_F64])
def test_every_float64_case_is_admitted(name, normalized):
    x, y, ref = F64.reference(name, normalized)
    fig = F64.compare(ref, F64.fp32_restatement(x, y, normalized))
    print(f"feature_nn f32 restatement {name} normalized={int(normalized)}: " + " ".join(f"{k}={v:.4g}" for k, v in fig.items()))
    assert fig["row_unclear"] <= C.UNCLEAR_CAP and fig["col_unclear"] <= C.UNCLEAR_CAP


def test_the_room_case_stays_out():
    x, y = C.build("1665x1700x3_room")
    ref = F64.brute_force(x, y, False)
    assert max((~ref["row_clear"]).mean(), (~ref["col_clear"]).mean()) > 0.2     # heavy cancellation: bits only


def test_comparison_refuses_planted_errors():
    x, y, ref = F64.reference("200x130x256_gauss", False)
    good = F64.fp32_restatement(x, y, False)
    F64.compare(ref, good)
    clear_row = int(np.nonzero(ref["row_clear"])[0][0])
    for k, change in ((0, lambda a: (a[clear_row] + 1) % 130), (1, lambda a: a[clear_row] * (1 + 1e-4)),
                      (2, lambda a: (a[clear_row] + 1) % 200), (3, lambda a: a[clear_row] + 1.0)):
        bad = [np.array(a) for a in good]
        assert ref["col_clear"][clear_row] or k < 2
        bad[k][clear_row] = change(bad[k])
        with pytest.raises(AssertionError):
            F64.compare(ref, bad)


def test_reduce_matrix_and_index_logic():
    d = np.array([[3, 1, 1, np.nan], [np.nan, np.nan, np.nan, np.nan], [0, 5, 0, 2]], np.float32)
    ri, rd, ci, cd = C.reduce_matrix(d)
    assert ri.tolist() == [1, 0, 0] and rd.tolist() == [1, np.inf, 0] and ci.tolist() == [2, 0, 2, 2] and cd.tolist() == [0, 1, 0, 2]
    ri, rd, ci, cd = C.reduce_matrix(np.zeros((2, 0), np.float32))
    assert ri.tolist() == [-1, -1] and np.isposinf(rd).all() and ci.shape == (0,)
    ref_nn, src_nn = np.array([1, 1, 0]), np.array([2, 0])
    assert [a.tolist() for a in C.reference_corr_indices(ref_nn, src_nn, 3, 2, False, False)] == [[0, 1, 2], [1, 1, 0]]
    assert [a.tolist() for a in C.reference_corr_indices(ref_nn, src_nn, 3, 2, True, False)] == [[0, 2], [1, 0]]
    assert [a.tolist() for a in C.reference_corr_indices(ref_nn, src_nn, 3, 2, False, True)] == [[0, 1, 2, 2, 0], [1, 1, 0, 0, 1]]


def test_golden_file_is_the_reference_logic(golden_dir):
    """tests/golden/feature_corr.npz (the reference's own functions on the host): no unclear decision, and its index arrays
    are the restated logic over the float64 neighbours."""
    import os
    g = np.load(os.path.join(golden_dir, "feature_corr.npz"))
    ref = F64.brute_force(g["ref_feats"], g["src_feats"], False)
    assert ref["row_clear"].all() and ref["col_clear"].all()
    n, m = g["ref_feats"].shape[0], g["src_feats"].shape[0]
    for tag, mutual, bilateral in (("plain", False, False), ("mutual", True, False), ("bilateral", False, True)):
        want = C.reference_corr_indices(ref["row_index"], ref["col_index"], n, m, mutual, bilateral)
        assert np.array_equal(g[tag + "_ref"], want[0]) and np.array_equal(g[tag + "_src"], want[1]), tag
    assert np.array_equal(g["corr_mutual_ref_points"], g["ref_points"][g["mutual_ref"]])

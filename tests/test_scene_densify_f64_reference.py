"""CPU: tests/scene_densify_f64.py (upstream's cat / mask sequence in float64) against a per-Gaussian Python loop written
from the definition in INTEGRATION.md: the emitted rows, their order, source, kind and every value to 1e-12; reset_opacity
the same way; and the committed seeds of the GPU test keep their margin from every threshold."""
import math

import pytest
import torch

import scene_densify_f64 as R

GPU_SIZES = [1, 63, 64, 65, 257, 1000, 4099]


def loop_reference(params, moments, stats, max_grad, min_opacity, extent, max_screen_size, percent_dense, noise):
    P = params["xyz"].shape[0]
    p64 = {n: p.to(torch.float64) for n, p in params.items()}
    blocks = ([], [], [], [])  # originals, clones, children 0, children 1: (source, {name: row})
    for i in range(P):
        d = int(stats[1][i])
        g = float(stats[0][i]) / d if d != 0 else 0.0
        sc = [float(v) for v in p64["scaling"][i]]
        s = max(math.exp(v) for v in sc)
        child_sc = [math.log(math.exp(v) / 1.6) for v in sc]
        s_child = max(math.exp(v) for v in child_sc)
        o = 1.0 / (1.0 + math.exp(-float(p64["opacity"][i, 0])))
        clone = g >= max_grad and s <= percent_dense * extent
        split = g >= max_grad and s > percent_dense * extent
        low = o < min_opacity
        screen = max_screen_size is not None
        big_r = screen and int(stats[2][i]) > max_screen_size
        big_w = screen and s > 0.1 * extent
        big_child = screen and s_child > 0.1 * extent
        row = {n: p[i] for n, p in p64.items()}
        if not (split or low or big_r or big_w):
            blocks[0].append((i, row))
        if clone and not low and not big_w:
            blocks[1].append((i, row))
        if split and not low and not big_child:
            r, x, y, z = [float(v) for v in p64["rotation"][i]]
            norm = math.sqrt(r * r + x * x + y * y + z * z)
            r, x, y, z = r / norm, x / norm, y / norm, z / norm
            rot = [[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                   [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                   [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]]
            for k in (0, 1):
                v = [math.exp(sc[c]) * float(noise[i, k, c]) for c in range(3)]
                child = dict(row)
                child["xyz"] = torch.tensor([float(p64["xyz"][i, a]) + sum(rot[a][c] * v[c] for c in range(3)) for a in range(3)],
                                            dtype=torch.float64)
                child["scaling"] = torch.tensor(child_sc, dtype=torch.float64)
                blocks[2 + k].append((i, child))
    source, kind, rows = [], [], []
    for k, block in enumerate(blocks):
        for i, row in block:
            source.append(i)
            kind.append(k)
            rows.append(row)
    out = {}
    for n, p in p64.items():
        out[n] = torch.stack([r[n] for r in rows]) if rows else p[:0]
    mom = {}
    for n, (m, v) in moments.items():
        pick = [(m[i].to(torch.float64), v[i].to(torch.float64)) if k == 0 else (torch.zeros_like(m[i], dtype=torch.float64),) * 2
                for i, k in zip(source, kind)]
        mom[n] = ([torch.stack([a for a, _ in pick]), torch.stack([b for _, b in pick])] if pick
                  else [m[:0].to(torch.float64), v[:0].to(torch.float64)])
    return out, mom, source, kind, tuple(len(b) for b in blocks)


@pytest.mark.parametrize("screen", [R.MAX_SCREEN, None])
@pytest.mark.parametrize("P,degree", [(1, 0), (65, 1), (257, 3)])
def test_sequence_equals_definition(P, degree, screen):
    params, moments, stats, noise = R.make_case(P, degree)
    args = (R.MAX_GRAD, R.MIN_OPACITY, R.EXTENT, screen, R.PERCENT_DENSE, noise)
    got = R.densify_and_prune(params, moments, stats, *args)
    want_p, want_m, source, kind, counts = loop_reference(params, moments, stats, *args)
    assert got["source"].tolist() == source and got["kind"].tolist() == kind
    assert got["counts"] == counts and got["P_new"] == len(source)
    if P >= 65:
        assert all(c > 0 for c in counts) and len(source) != P
    for n in params:
        assert got["params"][n].shape == want_p[n].shape, n
        assert torch.allclose(got["params"][n], want_p[n], rtol=1e-12, atol=1e-12), n
    assert sorted(got["moments"]) == sorted(moments) and "frozen" not in got["moments"]
    for n in moments:
        for a, b in zip(got["moments"][n], want_m[n]):
            assert torch.equal(a, b), n
    for z in got["stats"]:
        assert z.shape == (len(source),) and not z.any()


def test_reset_opacity():
    params, moments, _, _ = R.make_case(257, 0)
    new, mom = R.reset_opacity(params["opacity"], moments["opacity"])
    for i in range(257):
        o = min(1.0 / (1.0 + math.exp(-float(params["opacity"][i, 0]))), 0.01)
        assert abs(float(new[i, 0]) - math.log(o / (1.0 - o))) <= 1e-12 * abs(math.log(o / (1.0 - o)))
    assert not mom[0].any() and not mom[1].any()
    assert float(torch.sigmoid(new).max()) <= 0.01 * (1 + 1e-12)
    assert int((torch.sigmoid(new) < 0.0099).sum()) > 0  # the transparent fifth stays below the ceiling


@pytest.mark.parametrize("P", GPU_SIZES + [65859])
def test_committed_seeds_keep_their_margin(P):
    for degree in ([0, 1, 2, 3] if P < 65859 else [0]):
        params, _, stats, _ = R.make_case(P, degree)
        R.assert_margin(params, stats, R.MAX_GRAD, R.MIN_OPACITY, R.EXTENT, R.PERCENT_DENSE)


def test_margin_check_refuses_a_value_on_a_threshold():
    params, _, stats, _ = R.make_case(65, 0)
    params["scaling"][3] = math.log(R.PERCENT_DENSE * R.EXTENT * (1 + 1e-6))
    with pytest.raises(AssertionError):
        R.assert_margin(params, stats, R.MAX_GRAD, R.MIN_OPACITY, R.EXTENT, R.PERCENT_DENSE)

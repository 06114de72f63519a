"""The rasterizer's frame plan (gaussreg_amd/csrc/raster_plan.hpp: which launches count the tile instances of a frame, how the
counts reach the host, which scatter variant runs with how much LDS, how the count words decode) as plain host code: a
stand-alone driver (tests/raster_plan_driver.cpp) is built with the host compiler, once plainly and once with the address and
undefined-behaviour sanitizers, and fed plans to make.  No HIP, no GPU."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

COUNT_SCAN, TOTALS_SCAN, SELF_RAW = 0, 1, 2   # CountRoute
SYNC, EVENT, MAIL = 0, 1, 2                   # Transport
PLAIN, LATE, MANY = 0, 1, 2                   # PreprocessKind
SEG_READ, SEG_SELF_RAW, SEG_SELF_SCAN = 0, 1, 2
SEG_OF = {COUNT_SCAN: SEG_READ, TOTALS_SCAN: SEG_SELF_SCAN, SELF_RAW: SEG_SELF_RAW}
ROW = 2048  # SCAN_SINGLE_ROW = BIN_CHUNK


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("raster_plan_" + request.param) / "driver")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror"] + extra +
                   ["-I", os.path.join(ROOT, "gaussreg_amd", "csrc"), os.path.join(ROOT, "tests", "raster_plan_driver.cpp"),
                    "-o", exe], check=True)
    return exe


def ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


PS = [0, 1, 2047, 2048, 2049, 2048 * 2048, 2048 * 2048 + 1, 2 ** 31 - 2]
VS = [1, 2, 4, 5, 8, 32, 64]
IMAGES = [(16, 16), (640, 480), (2048, 128), (4080, 4080)]


def test_every_frame_gets_one_consistent_plan(driver):
    cases = list(itertools.product(PS, VS, IMAGES, *([(0, 1)] * 4)))
    got = ask(driver, ["plan %d %d %d %d %d %d %d %d" % (P, V, W, H, sh16, deferred, mailbox, bucket)
                       for P, V, (W, H), sh16, deferred, mailbox, bucket in cases])
    seen = set()
    for (P, V, (W, H), sh16, deferred, mailbox, bucket), o in zip(cases, got):
        ctx = (P, V, W, H, sh16, deferred, mailbox, bucket, o)
        gx, gy, tiles, nchunk, short_rows, preprocess, cam_in_args = o[:7]
        first, no_buckets, full_keys = o[7:13], o[13:19], o[19:25]
        assert (gx, gy, tiles, nchunk) == ((W + 15) // 16, (H + 15) // 16, ((W + 15) // 16) * ((H + 15) // 16),
                                           (P + ROW - 1) // ROW), ctx
        assert short_rows == int(nchunk <= ROW), ctx
        assert preprocess == (LATE if sh16 and V == 1 else MANY if bucket and V > 4 else PLAIN), ctx
        for plan, wants_buckets, key_bits in ((first, bucket, 27), (no_buckets, 0, 27), (full_keys, 0, 32)):
            route, transport, seg_mode, msd, totals_sorted, bits = plan
            assert route in (COUNT_SCAN, TOTALS_SCAN, SELF_RAW) and transport in (SYNC, EVENT, MAIL), ctx  # one of each
            assert (msd, bits) == (wants_buckets, key_bits), ctx
            if route == SELF_RAW:
                assert deferred and mailbox and msd and short_rows and V <= 4, ctx
            assert (route == COUNT_SCAN) == bool(short_rows and V <= 4 and route != SELF_RAW), ctx
            assert route == SELF_RAW or not (deferred and mailbox and msd and short_rows and V <= 4), ctx
            assert seg_mode == SEG_OF[route], ctx
            if not deferred:
                assert transport == SYNC, ctx
            else:
                # the counting kernels that mail are seg_scan_kernel<true> (CountScan) and the SEG_SELF_RAW scatter
                assert transport == (MAIL if mailbox and route != TOTALS_SCAN else EVENT), ctx
            if totals_sorted:
                assert V > 4 and msd, ctx
            assert totals_sorted == int(V > 4 and msd), ctx
        if cam_in_args:
            assert first[1] == MAIL and sh16 and V == 1 and deferred, ctx
        assert cam_in_args == int(bool(sh16 and V == 1 and deferred and mailbox and short_rows)), ctx
        seen.add((first[0], first[1]))
    # every pair the table of DESIGN.md 3.3 lists, and no other
    assert seen == {(COUNT_SCAN, SYNC), (COUNT_SCAN, EVENT), (COUNT_SCAN, MAIL), (TOTALS_SCAN, SYNC), (TOTALS_SCAN, EVENT),
                    (SELF_RAW, MAIL)}


def _scatter_expected(tiles, V, hint, spec):
    """The arithmetic of the scatter's LDS as the render call had it before the plan existed."""
    wide = V <= 4 and 16 * tiles * 4 <= 100 * 1024
    threads = 1024 if wide else 256
    cur = threads // 64 * ((tiles + 1) & ~1) * 2
    budget = 156 * 1024 if wide else 160 * 1024 // 6 - 512
    if budget < cur + 8 * 1024:
        budget = 78 * 1024
    cap_max = (budget - cur) // 2
    want = max(hint, 0)
    if spec:
        want = want + 64 if want > 0 else cap_max
    stage_cap = min(max(cap_max, 0), (want + 63) // 64 * 64)
    base = cur + (2 * stage_cap + 3) // 4 * 4
    elist = 1024 if tiles >= 4096 and base + threads // 64 * 1024 * 4 <= 156 * 1024 else 0
    return [threads, cur, max(cap_max, 0), stage_cap, elist, base + threads // 64 * elist * 4]


def test_scatter_plan_fits_the_lds(driver):
    # tile counts up to the largest the preprocess accepts (four cursor rows of 32-bit words in 156 KB), and both sides of
    # the limits of the wide workgroup (1 600 tiles) and of the per-wave instance list (4 096 tiles)
    TILES = [1, 2, 1024, 1200, 1600, 1601, 4095, 4096, 4097, 7000, 9984]
    HINTS = [-1, 0, 1, 63, 64, 65, 5000, 8533, 8597, 8598, 60672, 60673, 2 ** 31]
    cases = list(itertools.product(TILES, VS, HINTS, (0, 1)))
    got = ask(driver, ["scatter %d %d %d %d" % c for c in cases])
    for c, o in zip(cases, got):
        tiles, V, hint, spec = c
        threads, cur_bytes, stage_max, stage_cap, elist_cap, lds = o
        assert o == _scatter_expected(*c), (c, o)
        assert lds <= 160 * 1024 - 512, (c, o)
        assert 0 <= stage_cap <= stage_max, (c, o)
        # the hint is rounded up to whole waves; a hint past what the LDS allows gets exactly what it allows
        assert stage_cap % 64 == 0 or stage_cap == stage_max, (c, o)
        assert elist_cap in (0, 1024) and (elist_cap == 0 or tiles >= 4096), (c, o)
        assert lds == cur_bytes + (2 * stage_cap + 3) // 4 * 4 + threads // 64 * elist_cap * 4, (c, o)


def test_scatter_plan_anchor_values_at_640_by_480(driver):
    many, few = ask(driver, ["scatter 1200 5 %d 0" % 2 ** 31, "scatter 1200 4 %d 0" % 2 ** 31])
    assert many[:3] == [256, 9600, (163840 // 6 - 512 - 9600) // 2] and many[2] == 8597 and many[3] == 8597
    assert few[:3] == [1024, 38400, (159744 - 38400) // 2] and few[2] == 60672 and few[3] == 60672
    for hint, cap in ((1, 64), (8500, 8512), (8533, 8576), (8577, 8597)):   # min(cap, hint rounded up to 64)
        assert ask(driver, ["scatter 1200 32 %d 0" % hint])[0][3] == cap
    assert ask(driver, ["scatter 1200 1 0 1"])[0][3] == 60672       # speculative, no hint: all there is
    assert ask(driver, ["scatter 1200 1 3000 1"])[0][3] == 3072     # speculative: last frame's figure + 64, rounded up


def _layouts(totals, maxima, short_rows, far_words, seq):
    """One set of counts as the copied words (Sync, Event) and the mailed words (short rows only: long rows are not mailed)."""
    V = len(totals)
    per_view = maxima if short_rows else [-7] * V   # long rows: the scan leaves no per-view maxima; the words are not read
    out = {}
    for transport in (SYNC, EVENT):
        out[transport] = totals + per_view + [far_words[transport]] + ([] if short_rows else [max(maxima)])
    if short_rows:
        out[MAIL] = totals + per_view + [far_words[MAIL]] + [seq] * V
    return out


@pytest.mark.parametrize("V", [1, 5])
@pytest.mark.parametrize("short_rows", [1, 0])
def test_count_words_decode_alike_in_every_layout(driver, V, short_rows):
    totals = [1000003 * (v + 1) for v in range(V)]
    maxima = [40000 + 17 * ((3 * v) % V) for v in range(V)]   # the largest is not the first
    seq = 4711
    # (far depth, bucket overflow) -> the far word of each transport
    FAR = {(0, 0): {SYNC: 0, EVENT: 0, MAIL: 0}, (1, 0): {SYNC: 1, EVENT: 1, MAIL: seq}, (1, 1): {SYNC: 3, EVENT: -1, MAIL: -seq}}
    for (far, overflow), far_words in FAR.items():
        lay = _layouts(totals, maxima, short_rows, far_words, seq)
        got = ask(driver, ["decode %d %d %d %d %d %s" % (V, short_rows, t, seq, len(w), " ".join(map(str, w)))
                           for t, w in sorted(lay.items())])
        for o in got:
            assert o == [max(maxima), far, overflow] + totals


def test_far_word_rules(driver):
    def decode(transport, far_word, seq=4711):
        return ask(driver, ["decode 1 1 %d %d 4 10 5 %d %d" % (transport, seq, far_word, seq)])[0][1:3]

    # a plain frame reads bits: 1 = a far depth, 2 = an overflowed bucket (the ordering is redone in place)
    assert [decode(SYNC, w) for w in (0, 1, 2, 3)] == [[0, 0], [1, 0], [0, 1], [1, 1]]
    # behind the event the word was cleared in front of the frame: anything in it is this frame's
    assert [decode(EVENT, w) for w in (0, 1, 4711, -1, -4711)] == [[0, 0], [1, 0], [1, 0], [1, 1], [1, 1]]
    # nobody clears the mailed word: only this frame's stamp counts
    assert [decode(MAIL, w) for w in (4711, -4711)] == [[1, 0], [1, 1]]
    assert [decode(MAIL, w) for w in (0, 1, -1, 4710, -4710, 4712, 2 ** 31 - 1, -2 ** 31)] == [[0, 0]] * 8
    assert decode(MAIL, 1, seq=1) == [1, 0] and decode(MAIL, -1, seq=1) == [1, 1]

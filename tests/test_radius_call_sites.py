"""The radius search's call-site memory (gaussreg_amd/csrc/radius_sites.hpp: which kernel a (radius, limit) site gets) as
plain host code: a stand-alone driver (tests/radius_sites_driver.cpp) is built with the host compiler and fed choose / report
sequences.  No HIP, no GPU.  The expected answers are the behaviour of the dispatch this header was cut out of."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RETRY = 256  # TQ_RETRY_AFTER
SLOTS = 64   # TQ_MEMO


def bits(radius, ulps=0):
    return struct.unpack("<I", struct.pack("<f", radius))[0] + ulps


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("radius_sites") / "driver")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "gaussreg_amd", "csrc"),
                    os.path.join(ROOT, "tests", "radius_sites_driver.cpp"), "-o", exe, "-pthread"], check=True)
    return exe


class Script:
    """A command sequence for one fresh driver process, with the answer expected of every `choose`."""

    def __init__(self):
        self.lines, self.want = [], []

    def choose(self, rb, limit, want, times=1):
        self.lines += [f"choose {rb} {limit}"] * times
        self.want += [want] * times

    def gave_up(self, rb, limit, net):
        self.lines.append(f"report {rb} {limit} {net} 1")

    def finished(self, rb, limit, net):
        self.lines.append(f"report {rb} {limit} {net} 0")

    def check(self, exe):
        r = subprocess.run([exe], input="\n".join(self.lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        got = r.stdout.split()
        assert len(got) == len(self.want)
        wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, self.want)) if g != w]
        assert not wrong, wrong[:5]


R = bits(0.0625)


def test_unknown_site_starts_on_32_and_a_finished_call_creates_nothing(driver):
    s = Script()
    s.choose(R, 40, "32")
    s.finished(R, 40, "32")
    s.finished(R, 40, "64")
    s.choose(R, 40, "32", times=2 * RETRY + 2)
    s.check(driver)


def test_limit_40_walks_all_four_levels(driver):
    s = Script()
    s.gave_up(R, 40, "32")
    s.choose(R, 40, "64")
    s.gave_up(R, 40, "64")
    s.choose(R, 40, "presel")
    s.gave_up(R, 40, "presel")
    s.choose(R, 40, "count_fill", times=RETRY)
    s.choose(R, 40, "presel", times=RETRY + 1)   # one level back, then 256 calls there
    s.choose(R, 40, "64")
    s.check(driver)


@pytest.mark.parametrize("limit", [89, -1, 57, 0])
def test_limits_without_pre_selection_skip_it_both_ways(driver, limit):
    s = Script()
    s.gave_up(R, limit, "32")
    s.choose(R, limit, "64")
    s.gave_up(R, limit, "64")
    s.choose(R, limit, "count_fill", times=RETRY)
    s.choose(R, limit, "64", times=RETRY + 1)    # the 257th call steps back two levels
    s.choose(R, limit, "32", times=RETRY + 2)
    s.check(driver)


def test_limit_56_is_the_last_with_pre_selection(driver):
    s = Script()
    s.gave_up(R, 56, "64")
    s.choose(R, 56, "presel")
    s.gave_up(R, 1, "64")
    s.choose(R, 1, "presel")
    s.check(driver)


def test_level_1_steps_back_after_256_calls_and_level_0_does_not_count(driver):
    s = Script()
    s.gave_up(R, 40, "32")
    s.choose(R, 40, "64", times=RETRY)
    s.choose(R, 40, "32", times=3 * RETRY)
    s.gave_up(R, 40, "32")                       # the site is still known: a report moves it again
    s.choose(R, 40, "64", times=RETRY)
    s.choose(R, 40, "32")
    s.check(driver)


def test_a_report_restarts_the_count_and_sets_the_level_from_the_kernel_that_ran(driver):
    s = Script()
    s.gave_up(R, 40, "32")
    s.choose(R, 40, "64", times=RETRY - 1)
    s.gave_up(R, 40, "32")                       # (the same kernel again: level 1, calls from 0)
    s.choose(R, 40, "64", times=RETRY)
    s.choose(R, 40, "32")
    s.gave_up(R, 40, "presel")
    s.choose(R, 40, "count_fill")
    s.gave_up(R, 40, "32")                       # not "one up from where the site is": one up from the kernel reported
    s.choose(R, 40, "64")
    s.check(driver)


def test_sites_are_keyed_by_radius_bits_and_limit(driver):
    s = Script()
    s.gave_up(R, 40, "32")
    s.choose(bits(0.0625, 1), 40, "32")
    s.choose(R, 41, "32")
    s.choose(R, -1, "32")
    s.choose(R, 40, "64")
    s.gave_up(bits(0.0625, 1), 40, "64")
    s.choose(bits(0.0625, 1), 40, "presel")
    s.choose(R, 40, "64")
    s.check(driver)


def test_eviction_is_round_robin_over_a_full_table(driver):
    s = Script()
    site = [bits(0.01 * (i + 1)) for i in range(SLOTS + 2)]
    for i in range(SLOTS):
        s.gave_up(site[i], 40, "32")
    for i in range(SLOTS):
        s.choose(site[i], 40, "64")
    s.finished(site[SLOTS], 40, "32")            # takes no slot
    s.choose(site[0], 40, "64")
    s.gave_up(site[SLOTS], 40, "32")             # the 65th site takes the first slot
    s.choose(site[0], 40, "32")
    s.choose(site[1], 40, "64")
    s.choose(site[SLOTS], 40, "64")
    s.gave_up(site[SLOTS + 1], 40, "32")         # the 66th the second
    s.choose(site[1], 40, "32")
    s.choose(site[2], 40, "64")
    s.choose(site[SLOTS], 40, "64")
    s.choose(site[SLOTS + 1], 40, "64")
    s.check(driver)

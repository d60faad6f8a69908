"""CPU unit test of the stage passes' host arithmetic (instantsfm_amd/csrc/stage_plan.h, used by csrc/tracks.hip,
covis.hip, pair_inliers.hip and passes.hip through stage_device.h): the radix sorts' key bits against their definition
and against what they are for (a sort on the low bits orders like a sort on the whole key), the grid sizes at their
edges, and the running maximum of hipcub's size queries.  tests/cpp/stage_plan_test.cpp answers one query per line in
integers, so every comparison is exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 1, 2, 3, every 2^k and 2^k +- 1 for k <= 40, and 2^62
NS = sorted({1, 2, 3, 1 << 62} | {(1 << k) + d for k in range(41) for d in (-1, 0, 1)})


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("stage_plan") / "stage_plan_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(REPO, "tests", "cpp", "stage_plan_test.cpp")], check=True)

    def run(queries):
        out = subprocess.run([exe], input="".join(q + "\n" for q in queries), check=True, capture_output=True,
                             text=True, timeout=120).stdout.splitlines()
        assert len(out) == len(queries)
        return [int(x) for x in out]
    return run


def bits_by_definition(n):
    """The smallest b in [1, 62] with 2^b >= n."""
    return next(b for b in range(1, 63) if (1 << b) >= n)


def test_bits_for_is_its_definition(ask):
    assert {0, 1, 2, 3, 255, 256, 257, (1 << 40) + 1, 1 << 62} <= set(NS) and len(NS) == 121
    got = ask([f"bits {n}" for n in NS])
    assert got == [bits_by_definition(n) for n in NS]
    assert got[NS.index(1)] == 1 and got[NS.index(257)] == 9 and got[-1] == 62


def test_sort_on_the_key_bits_is_the_sort_on_the_key(ask):
    """What too few bits would break: 1,000 keys in [0, n), stably sorted on their low bits_for(n) bits, come out in
    the order of the stable sort on the whole key."""
    ns = [n for n in NS if 1 <= n <= 1 << 20]
    assert ns[-1] == 1 << 20 and len(ns) == 58
    rng = np.random.default_rng(20)
    for n, b in zip(ns, ask([f"bits {n}" for n in ns])):
        keys = rng.integers(0, n, 1000, dtype=np.int64)
        if n > 1:
            keys[:2] = (0, n - 1)  # both ends of the range are always among them
        low = keys & ((1 << b) - 1)
        np.testing.assert_array_equal(np.argsort(low, kind="stable"), np.argsort(keys, kind="stable"), err_msg=str(n))


@pytest.mark.parametrize("per", [4, 256])
def test_blocks_for(ask, per):
    ns = [0, 1, per - 1, per, per + 1, (1 << 31) - 1]
    got = ask([f"blocks {n} {per}" for n in ns])
    assert got == [-(-n // per) for n in ns]
    assert got[:5] == [0, 1, 1, 1, 2] and got[5] == (1 << 31) // per


def test_temp_bytes_is_the_largest_query(ask):
    assert ask(["temp", "temp 0", "temp 7", "temp 3 9 4", "temp 9 3", "temp 1 2 3 4"]) == [0, 0, 7, 9, 9, 4]

"""GPU: the optimal-trading-rule mesh (csrc/fmk_otr.hip) on the kernel paths tests/test_gpu_otr.py does not
reach, against tests/_otr_ref.py, bit-equal on all seven outputs.  Every instantiation of k_otr_walk from both sides of the node
counts at which the dispatcher changes it, generated and through normals=; level lists that fill a side's records in one step or
switch a side off; long horizons with noise, with record steps above 2048 on both barriers, and paths steered through the last
pair of 4096 steps; and a call whose partials pass the cap, so that it goes out in two launches.  The cases are built in
tests/test_otr_host.py, which asserts on the reference alone that they hold what they are there for."""
import time

import numpy as np
import pytest

from tests import _otr_ref as R
from tests.test_gpu_otr import assert_same, run
from tests.test_otr_host import (EDGE_CASES, EDGE_LEVEL_KINDS, EDGE_LEVEL_SHAPES, EDGE_NORMALS, EDGE_SHAPES, FIELDS, LONG_HP, SPLIT_CFG,
                                 SPLIT_PERIOD, edge_reference, long_steer_case, long_steer_node00, npl_of, one_set, reference, shape_of,
                                 split_case, split_cpl)

pytestmark = pytest.mark.gpu


def of_set(mesh, c):
    return {k: getattr(mesh, k)[c:c + 1] for k in FIELDS}


# ---------------------------------------------------------------------------------------------- A: every instantiation of the walk
@pytest.mark.parametrize("name", list(EDGE_SHAPES))
def test_every_walk_from_both_sides_of_its_boundaries(name):
    got = run(EDGE_CASES[name])
    assert got.sharpe.shape == (1,) + EDGE_SHAPES[name]
    assert_same(got, edge_reference(name), (name, "NPL", npl_of(got.sharpe[0].size)))


@pytest.mark.parametrize("name", [n if hp == 24 else f"{n} max_hp 25" for hp in (24, 25) for n in EDGE_NORMALS] + ["5x13 open max_hp 25"])
def test_given_normals_equal_the_generated_ones(name):
    case = EDGE_CASES[name]
    assert npl_of(len(case["pt"]) * len(case["sl"])) > 1
    seeded = run(case)
    given = run(case, R.normals(case["seed"], case["n_paths"], case["max_hp"]))
    assert_same(given, seeded, name)
    assert_same(given, edge_reference(name), name)


@pytest.mark.parametrize("kind", EDGE_LEVEL_KINDS)
@pytest.mark.parametrize("name", EDGE_LEVEL_SHAPES)
def test_level_lists_that_fill_or_switch_off_a_side(name, kind):
    got = run(EDGE_CASES[f"{name} {kind}"])
    assert got.sharpe.shape == (1,) + shape_of(name)
    assert_same(got, edge_reference(f"{name} {kind}"), (name, kind))


def test_parameter_sweep_on_a_non_square_mesh():
    case = EDGE_CASES["sweep"]
    got = run(case)
    assert_same(got, edge_reference("sweep"))
    for c in range(len(case["forecast"])):
        assert_same(of_set(got, c), run(one_set(case, c)), c)


# ---------------------------------------------------------------------------------------------- B: long horizons
@pytest.mark.parametrize("max_hp", LONG_HP)
def test_long_horizons_with_noise(max_hp):
    assert_same(run(EDGE_CASES[f"long {max_hp}"]), edge_reference(f"long {max_hp}"), max_hp)


@pytest.mark.parametrize("max_hp", [4095, 4096])
def test_paths_steered_through_the_last_pair(max_hp):
    case, z = long_steer_case(max_hp)
    got = run(case, z)
    assert_same(got, reference(case, z), max_hp)
    node = tuple(int(getattr(got, k)[0, 0, 0]) for k in ("hold", "n_profit", "n_stop", "n_time"))
    assert node == long_steer_node00(max_hp) and node[1:] == (32, 24, 16)


# ---------------------------------------------------------------------------------------------- C: a call split into launches
def test_a_call_split_into_two_launches():
    case = split_case()
    cpl = split_cpl(case)
    assert 1 < cpl < SPLIT_CFG <= 2 * cpl
    t0 = time.perf_counter()
    got = run(case)
    print(f"{SPLIT_CFG} sets, sets per launch {cpl}: {time.perf_counter() - t0:.3f} s for the call")
    first = {k: getattr(got, k)[:SPLIT_PERIOD] for k in FIELDS}
    for c0 in range(0, SPLIT_CFG, SPLIT_PERIOD):                         # set c is set c % 61: every set of both launches
        n = min(SPLIT_PERIOD, SPLIT_CFG - c0)
        assert_same({k: getattr(got, k)[c0:c0 + n] for k in FIELDS}, {k: v[:n] for k, v in first.items()}, c0)
    for c in (0, cpl - 1, cpl, SPLIT_CFG - 1):
        assert_same(of_set(got, c), run(one_set(case, c)), c)
    for c in (cpl - 1, cpl):
        assert_same(of_set(got, c), reference(one_set(case, c)), c)
    assert not np.array_equal(got.mean[cpl - 1], got.mean[cpl])

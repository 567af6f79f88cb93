"""The coarsest-level direct solvers (csrc/coarse.hip, dense.hip, sine_cube16.h) at the edges of every path, against the
refined reference of tests/coarse_cases.py.  Needs an MI355X.

fp64: error <= 8 x max(the case's yardstick error, 2^-53 kappa_1(A)) relative to max|x| (coarse_cases.bound64; the 8 is a
supposition, not a measurement).  fp32, sine paths (computed in double, rounded once): componentwise
|x32 - x_ref(b32)| <= 2^-24 |x_ref| + the fp64 bound (derived).  fp32, the products with a stored inverse:
8 x max(fp32 yardstick error, 2^-24 kappa_1(A)).  No bound is fitted to device output; every case prints its figures
(`coarse-edge ...`; the table of a run: profiles/coarse_edges.txt)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coarse_cases as cc
from coarse_edges_worker import DTYPES, solve_on_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def report_and_check(case, dtype, info, x, route=""):
    """print the case's line, then assert: the path that answered, and the bound"""
    num = cc.numbers(case)
    sine32 = dtype == "float32" and info["blocks"] == 0
    if dtype == "float64":
        dev, yard, unit, bound = cc.error(x, num.ref), num.yard_err, cc.U64 * num.kappa, cc.bound64(num)
        ratio = dev / max(yard, unit)
    elif sine32:
        allow = cc.sine32_allowance(num)
        hi, lo = num.ref32
        diff = np.abs((x.astype(cc.LD) - hi.astype(cc.LD)) - lo.astype(cc.LD)).astype(np.float64)
        dev, yard, unit, bound = cc.error(x, num.ref32), num.yard_b32_err, cc.U32, None
        ratio = float((diff / allow).max())                   # componentwise: must be <= 1
    else:
        dev, yard, unit, bound = cc.error(x, num.ref32), num.yard32_err or 0.0, cc.U32 * num.kappa, cc.bound32(num)
        ratio = dev / max(yard, unit)
    print("coarse-edge %-28s %-7s %sblocks %2d n %5d kappa1 %.2e  device %.3e  yardstick %.3e  unit %.3e  device/yardstick %s  device/max(yardstick, unit) %.3f%s"
          % (case.name, dtype, route, info["blocks"], info["n"], num.kappa, dev, yard, unit, "%.2f" % (dev / yard) if yard > 0 else "-", ratio,
             "  (componentwise, of the allowance: <= 1)" if sine32 else "  (<= 8)"))
    assert info["n"] == num.n
    assert info["blocks"] == case.blocks, "the path that answered is not the one the case is about"
    assert np.all(np.isfinite(x))
    if sine32:
        assert np.all(diff <= allow), "worst component at %.3f of its allowance" % ratio
    else:
        assert dev <= bound, "%.3e against %.3e" % (dev, bound)


def run(case, dtype):
    num = cc.numbers(case)
    info, x = solve_on_device(case, num, dtype, num.b if dtype == "float64" else num.b32)
    report_and_check(case, dtype, info, x)
    return info


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", cc.sine_cases(), ids=repr)
def test_sine_transform_solve(case, dtype):
    """E = 16 / 32 on both sides of a largest extent of 16 / 17 and at 32, every slot of a thread live (n > 7168), n = 8192
    itself, more than 64 KB of LDS, more than 256 lines in a pass, single-k-step extents, n = 2 — Poisson and anisotropic
    couplings; two shapes that must leave the path for the explicit inverse"""
    info = run(case, dtype)
    if case.blocks == 0:
        ext = tuple(case.extents) + (1, 1)
        assert info["half_bandwidth"] == ext[0] * ext[1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", cc.inverse_cases(), ids=repr)
def test_explicit_inverse(case, dtype):
    """either side of the pivoted / blocked switch (256), of the 64-row tiles, of the mat-vec's 16-byte loads; zero tiles
    of narrow and tile-cutting bands and on one side only; in-block pivoting that succeeds"""
    run(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", cc.growth_cases(), ids=repr)
def test_blocked_inverse_under_growth(case, dtype):
    """operators on which elimination without pivoting across blocks grows: whichever route answers (the blocked one if its
    acceptance check lets it, the pivoted one otherwise), the yardstick bound holds"""
    run(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", cc.nullspace_cases(), ids=repr)
def test_regularised_inverse_through_the_blocked_route(case, dtype):
    """nullspace='constant' with 294 and 512 unknowns on the coarsest level: A + gamma 1 1^T through the blocked
    elimination; the reference solves the regularised system (= pinv(A) b + mean(b) / (gamma n))"""
    run(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", cc.substructuring_cases(), ids=repr)
def test_substructuring(case, dtype):
    """P = 2 and the maximum 64, blocks exactly 2 w long, the largest P the rule admits on 40 x 40, unsymmetric band"""
    run(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", cc.chain_cases(), ids=repr)
def test_block_chain(case, dtype):
    """bs equal to the half-bandwidth, K = 2, a last block of one row, bs = 1"""
    run(case, dtype)


PIVOTED = ("inverse-dense-256", "inverse-dense-321")


def test_pivoted_elimination_at_blocked_sizes():
    """OMG_DENSE_BLOCKED=0 is read once per process: one child (tests/coarse_edges_worker.py) solves both cases in both
    precisions with the column-by-column elimination; the bounds are checked here"""
    env = dict(os.environ, OMG_DENSE_BLOCKED="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    child = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "coarse_edges_worker.py")] + list(PIVOTED), env=env, capture_output=True,
                           text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-3000:]
    out = json.loads(child.stdout.strip().splitlines()[-1])
    cases = {c.name: c for c in cc.inverse_cases()}
    for name in PIVOTED:
        for dtype in DTYPES:
            report_and_check(cases[name], dtype, out[name][dtype]["info"], np.array(out[name][dtype]["x"]), route="pivoted ")

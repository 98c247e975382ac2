"""Which headwaters the in-pass may route (rr_plan.hpp: mark_inpass_headwaters), without a GPU: the count on a small fixed forest, and the
coefficient rule -- c1row is +0.0 and c2 is finite, both on the bits -- that lets k_rec_in evaluate fma(c1row, 0.0, fma(c2, 0.0, r)) as
r + 0.0.  A headwater's c1row cannot be set through the C ABI, so the rule is exercised on the planner's own function by a small
stand-alone program (inpass_eligibility_main.cpp, compiled with rr_plan.cpp); a non-finite c2 through the ABI is in test_gpu_inpass_walk.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from river_route_amd._lib import RR_DEVICE_NONE
from river_route_amd.engine import Plan
from test_gpu_inpass_walk import N, csc_from_down, forest, headwaters

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_count_on_the_fixed_forest():
    """70 reaches, 24 headwaters, none mirrored, no wide tile: 24 eligible -- what the plan reported before the rule looked at coefficients."""
    down = forest()
    indptr, indices = csc_from_down(down)
    assert headwaters(down).size == 24
    with Plan(indptr, indices, device=RR_DEVICE_NONE) as plan:
        hw = plan.inpass_info()
    assert hw == {'enabled': hw['enabled'], 'eligible': 24, 'headwater_positions': 24, 'mirrored_or_boundary': 0, 'wide_tile': 0}
    assert N == 70


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler on the path'
    exe = str(tmp_path_factory.mktemp('inpass_eligibility') / 'inpass_eligibility')
    subprocess.run([cxx, '-std=c++17', '-O0', '-o', exe, os.path.join(HERE, 'inpass_eligibility_main.cpp'),
                    os.path.join(ROOT, 'river_route_amd', 'csrc', 'rr_plan.cpp')], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60)
    return {line.split()[0]: line.split()[1:] for line in r.stdout.splitlines()}


def test_structure_alone_without_coefficients(program):
    """Reaches 0..8 are headwaters, reach 9 has an upstream reach: nine eligible while the plan has no coefficients."""
    assert program['structure'] == ['1111111110', '9', '9', '9']


def test_plain_coefficients_change_nothing(program):
    assert program['plain'] == ['1111111110', '9', '9', '9']


def test_non_finite_c2_or_other_c1row_is_not_eligible(program):
    """Reach 0: c2 +inf, 1: -inf, 2: NaN, 3: c1row -0.0, 4: c1row 1.0 -- left to k_tile; 5: c2 negative, 6: subnormal, 7: -0.0, 8: c3 inf -- eligible.
    They stay headwater positions (the last figure)."""
    assert program['odd'] == ['0000011110', '4', '4', '9']

"""The one derivation of the coefficient tables (rr_plan.hpp: tributary_weight, lag_coef, reach_coef, tile_coef and its masked forms),
without a GPU.  coef_tables_main.cpp, compiled with rr_plan.cpp -- once plainly, once under AddressSanitizer + UndefinedBehaviorSanitizer
(the program links the sanitizer itself) -- reads a case file and prints every table as 64-bit words; both executables run every case and
must print the same.  The tables are compared on their BIT PATTERNS with a numpy restatement of the definitions, which takes its layout
arrays from a host-only Plan (layout(), tile_layout(), direct_layout()), never from the functions under test."""
import contextlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from river_route_amd import synth
from river_route_amd._lib import RR_DEVICE_NONE
from river_route_amd.engine import Plan
from test_gpu_inpass_walk import csc_from_down, forest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TILE_GHOST, TILE_EXPORT, DIRECT_HOLE = 1 << 28, 1 << 27, 1 << 30      # rr_plan.hpp: kTileGhost, kTileExport, kDirectHole
DIRECT_LANES, DIRECT_WMAX = 256, 62                                    # what rr_plan_create hands build_direct_plan


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@contextlib.contextmanager
def tile_block(block):
    """The tile capacity is read from the environment when a plan is made."""
    old = {k: os.environ.pop(k, None) for k in ('RR_TILE_BLOCK', 'RR_DIRECT', 'RR_HW_INPASS')}
    os.environ['RR_TILE_BLOCK'] = str(block)
    try:
        yield
    finally:
        del os.environ['RR_TILE_BLOCK']
        os.environ.update({k: v for k, v in old.items() if v is not None})


class Layouts:
    """The layout arrays of a host-only plan."""

    def __init__(self, indptr, indices, block):
        self.indptr, self.indices, self.block = np.asarray(indptr, np.int32), np.asarray(indices, np.int32), block
        self.n = self.indptr.size - 1
        with tile_block(block), Plan(self.indptr, self.indices, device=RR_DEVICE_NONE) as plan:
            self.perm, self.lag, self.child_ptr = plan.layout()
            self.tile_info, self.direct_info, self.inpass_info = plan.tile_info(), plan.direct_info(), plan.inpass_info()
            self.tile = plan.tile_layout()
            self.direct = plan.direct_layout() if self.direct_info['ok'] else None


def restate(L, lhs, c2, c3, c4, ghosts=()):
    """Every table from the definitions: {name: array}, float64 tables and int64 words."""
    n = L.n
    has_edge = L.indptr[1:] > L.indptr[:-1]

    def weight(reaches):      # minus the lhs_off_data entry of the edge leaving each reach, 0.0 at an outlet
        reaches = np.asarray(reaches)
        w = np.zeros(reaches.shape)
        e = has_edge[reaches]
        if e.any():
            w[e] = -lhs[L.indptr[reaches[e]]]
        return w
    c1row, differ = np.zeros(n), -1
    for p in range(n):
        ups = L.perm[L.child_ptr[p]:L.child_ptr[p + 1]]      # the upstream reaches in child_ptr's order
        if ups.size:
            w = weight(ups)
            c1row[L.perm[p]] = w[0]
            if (w[1:] != w[0]).any():
                differ = int(L.perm[p]) if differ < 0 else min(differ, int(L.perm[p]))
    reach = np.stack([c1row, c2, c3, np.zeros(n) if c4 is None else c4], axis=1)
    out = {'differ': np.array([differ]), 'reach': reach, 'member_c1row': c1row, 'w': weight(L.perm)}
    for k, name in enumerate(('c1row', 'c2', 'c3', 'c4')):
        out[name] = reach[L.perm, k]

    t = L.tile
    npos = t['perm'].size
    ghost = (t['lag'] & TILE_GHOST) != 0
    own = np.flatnonzero(~ghost)
    inv = np.full(n, -1)
    inv[t['perm'][own]] = own
    assert (inv >= 0).all()
    tile = np.zeros((npos, 3))
    tile[own] = reach[t['perm'][own], :3]
    out['tile_no_list'] = tile.copy()
    tile[inv[list(ghosts)]] = 0.0
    out['tile'] = out['tile_dense'] = tile
    # the in-pass headwaters (rr_plan.hpp: mark_inpass_headwaters)
    ups_in_tile = t['ccnt'] & 0xFFFF
    tile_of = np.searchsorted(t['tile_ptr'], np.arange(npos), side='right') - 1
    wide = np.array([(ups_in_tile[t['tile_ptr'][k]:t['tile_ptr'][k + 1]] > 3).any() for k in range(t['tile_ptr'].size - 1)])
    boundary = np.zeros(npos, bool)
    boundary[inv[list(ghosts)]] = True
    elig = (~ghost & (ups_in_tile == 0) & ((t['lag'] & TILE_EXPORT) == 0) & ~boundary & ~wide[tile_of]
            & (bits(tile[:, 0]) == 0) & np.isfinite(tile[:, 1]))
    out['elig'] = elig.astype(np.int64)
    out['tile_hw'] = np.where(elig[:, None], 0.0, tile)
    out['tile_unit'] = np.where((ups_in_tile == 0)[:, None], 0.0, tile)
    out['col'] = tile[inv]
    if L.direct is not None:
        holes = np.flatnonzero(L.direct['delay'] & DIRECT_HOLE)
        skel = np.zeros((L.direct_info['skeleton_positions'], 3))
        skel[L.direct['xinfo'][holes]] = reach[holes, :3]      # every other position of the skeleton is a ghost
        out['skel'] = skel
    return out


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler on the path'
    d = tmp_path_factory.mktemp('coef_tables')
    exes = []
    for name, flags in (('plain', ['-O2']), ('sanitized', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exes.append(str(d / name))
        subprocess.run([cxx, '-std=c++17', *flags, '-o', exes[-1], os.path.join(HERE, 'coef_tables_main.cpp'),
                        os.path.join(ROOT, 'river_route_amd', 'csrc', 'rr_plan.cpp')], check=True, capture_output=True, text=True, timeout=300)
    return d, exes


def run_case(programs, L, sets, ghosts=()):
    """sets: [(lhs or None, c2, c3, c4 or None)].  Returns {name: uint64 words} as both executables print it."""
    d, exes = programs

    def words(a):
        return ' '.join(f'{int(v):016x}' for v in bits(a))
    text = [f'{L.n} {L.indices.size} {L.block} {min(DIRECT_LANES, L.block)} {DIRECT_WMAX}', ' '.join(map(str, L.indptr)), ' '.join(map(str, L.indices)),
            ' '.join(map(str, [len(ghosts), *ghosts])), str(len(sets))]
    for lhs, c2, c3, c4 in sets:
        text += [f'{int(lhs is not None)} {int(c4 is not None)}'] + [words(a) for a in (lhs, c2, c3, c4) if a is not None]
    path = d / 'case.txt'
    path.write_text('\n'.join(text) + '\n')
    outs = []
    for exe in exes:
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == '', f'{exe}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'
        outs.append(r.stdout)
    assert outs[0] == outs[1], 'the sanitized build prints other tables'
    return {ln.split()[0]: np.array([int(w, 16) for w in ln.split()[1:]], dtype=np.uint64) for ln in outs[0].splitlines()}


def assert_tables(got, want, s=0):
    """Every table of set s on the bits."""
    for name, a in want.items():
        g = got[f'{s}.{name}']
        w = a.astype(np.int64).view(np.uint64) if a.dtype.kind == 'i' else bits(a).ravel()
        assert g.shape == w.shape and np.array_equal(g, w), f'table {name} of set {s}: first difference at word {np.flatnonzero(g != w)[:1] if g.shape == w.shape else "shape"}'


def distinct(n, seed=0):
    """(c1, c2, c3, c4): every value of every array differs from every other."""
    i = np.arange(n, dtype=np.float64) + 10 * seed
    return 0.11 + 0.003 * i, 0.21 + 0.005 * i, 0.31 + 0.007 * i, 0.41 + 0.011 * i


def coeff_set(L, seed=0):
    c1, c2, c3, c4 = distinct(L.n, seed)
    return -c1[L.indices], c2, c3, c4


@pytest.fixture(scope='module')
def base():
    net = synth.synth_network(60, seed=1, order='postorder')
    return Layouts(*csc_from_down(net.down_index), block=32)


def test_base_every_table(programs, base):
    L = base
    assert (L.tile_info['tiles'], L.tile_info['ghosts']) == (3, 4)
    assert L.direct_info['ok'] and (L.direct_info['skeleton_positions'], L.direct_info['holes']) == (8, 4)
    assert (L.inpass_info['headwater_positions'], L.inpass_info['eligible']) == (30, 29)
    sets = [coeff_set(L)]
    got = run_case(programs, L, sets)
    want = restate(L, *sets[0])
    assert list(got['info'].astype(np.int64)) == [L.tile_info['positions'], 4, 3, L.tile_info['levels'], 1, 8, 4]
    assert want['differ'][0] == -1 and want['elig'].sum() == 29
    assert_tables(got, want)
    assert np.array_equal(got['members'], got['0.tile'])


def test_forest_every_table(programs):
    L = Layouts(*csc_from_down(forest()), block=8)
    assert (L.tile_info['tiles'], L.tile_info['ghosts'], L.tile_info['levels']) == (14, 29, 10) and not L.direct_info['ok']
    sets = [coeff_set(L)]
    got = run_case(programs, L, sets)
    assert list(got['info'].astype(np.int64))[:5] == [L.tile_info['positions'], 29, 14, 10, 0]
    assert_tables(got, restate(L, *sets[0]))
    assert '0.skel' not in got


def test_single_reach_without_edges(programs):
    L = Layouts(np.array([0, 0]), np.array([], np.int32), block=32)
    c2, c3, c4 = np.array([0.25]), np.array([0.5]), np.array([0.125])
    got = run_case(programs, L, [(None, c2, c3, c4)])
    assert_tables(got, restate(L, None, c2, c3, c4))
    assert np.array_equal(got['0.reach'], bits([0.0, 0.25, 0.5, 0.125]))


def test_signed_zeros_keep_their_sign(programs, base):
    """lhs_off_data +0.0 gives c1row -0.0 and the other way round: on the bits, in every table that carries c1row."""
    L = base
    lhs, c2, c3, c4 = coeff_set(L)
    inner = [int(L.perm[p]) for p in range(L.n) if L.child_ptr[p + 1] > L.child_ptr[p]]
    a, b = inner[0], inner[-1]
    lhs = lhs.copy()
    lhs[L.indices == a] = 0.0
    lhs[L.indices == b] = -0.0
    got = run_case(programs, L, [(lhs, c2, c3, c4)])
    want = restate(L, lhs, c2, c3, c4)
    assert_tables(got, want)
    reach = got['0.reach'].reshape(L.n, 4)
    assert reach[a, 0] == 0x8000000000000000 and reach[b, 0] == 0
    own = np.flatnonzero((L.tile['lag'] & TILE_GHOST) == 0)
    tile = got['0.tile'].reshape(-1, 3)
    assert tile[own[L.tile['perm'][own] == a], 0] == 0x8000000000000000 and tile[own[L.tile['perm'][own] == b], 0] == 0
    assert want['differ'][0] == -1      # (+0.0 and -0.0 are equal weights)


def test_a_reach_with_two_different_weights_is_reported(programs, base):
    L = base
    lhs, c2, c3, c4 = coeff_set(L)
    inv = np.argsort(L.perm)
    two = [p for p in range(L.n) if L.child_ptr[p + 1] - L.child_ptr[p] == 2]
    p = two[len(two) // 2]
    reach, second = int(L.perm[p]), int(L.perm[L.child_ptr[p] + 1])
    lhs = lhs.copy()
    lhs[L.indptr[second]] *= 0.5
    got = run_case(programs, L, [(lhs, c2, c3, c4)])
    want = restate(L, lhs, c2, c3, c4)
    assert want['differ'][0] == reach and got['0.differ'].astype(np.int64)[0] == reach
    assert_tables(got, want)
    w = got['0.w'].view(np.float64)      # the streaming kernel's per-edge weights carry both
    first = int(L.perm[L.child_ptr[p]])
    assert w[inv[first]] == -lhs[L.indptr[first]] and w[inv[second]] == -lhs[L.indptr[second]] and w[inv[first]] != w[inv[second]]


def test_boundary_ghosts_get_zeros_and_nothing_else_changes(programs, base):
    L = base
    sets = [coeff_set(L)]
    heads = [int(L.perm[p]) for p in range(L.n) if L.child_ptr[p + 1] == L.child_ptr[p]]
    ghosts = (heads[3], heads[17])
    got = run_case(programs, L, sets, ghosts)
    want = restate(L, *sets[0], ghosts=ghosts)
    assert_tables(got, want)
    tile, plain = got['0.tile'].reshape(-1, 3), got['0.tile_no_list'].reshape(-1, 3)
    own = np.flatnonzero((L.tile['lag'] & TILE_GHOST) == 0)
    at = np.isin(np.arange(tile.shape[0]), [own[L.tile['perm'][own] == g][0] for g in ghosts])
    assert at.sum() == 2 and (tile[at] == 0).all() and (plain[at, 1:] != 0).all() and np.array_equal(tile[~at], plain[~at])
    # tile_coef is a function of the set and the list alone (here: the list in the other order); which setter came first cannot matter to it
    assert np.array_equal(got['0.tile'], run_case(programs, L, sets, ghosts[::-1])['0.tile'])
    assert not want['elig'][at].any() and np.array_equal(got['0.col'].reshape(L.n, 3)[list(ghosts)], np.zeros((2, 3), np.uint64))


def test_two_members_each_get_the_table_of_their_own_arrays(programs, base):
    L = base
    sets = [coeff_set(L, 0), coeff_set(L, 1)]
    got = run_case(programs, L, sets)
    slices = got['members'].reshape(2, -1)
    for m in range(2):
        want = restate(L, *sets[m])
        assert_tables(got, want, m)
        assert np.array_equal(slices[m], bits(want['tile']).ravel())
        assert np.array_equal(slices[m], run_case(programs, L, [sets[m]])['0.tile'])      # the single-set table of its own arrays
    assert not np.array_equal(slices[0], slices[1])


def test_without_c4_dt_the_fourth_column_is_zero(programs, base):
    L = base
    lhs, c2, c3, _ = coeff_set(L)
    got = run_case(programs, L, [(lhs, c2, c3, None)])
    assert_tables(got, restate(L, lhs, c2, c3, None))
    assert (got['0.reach'].reshape(L.n, 4)[:, 3] == 0).all() and (got['0.c4'] == 0).all()
    assert (got['0.reach'].reshape(L.n, 4)[:, :3] != 0).any(axis=0).all()

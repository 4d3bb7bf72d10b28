"""The jump-ahead of doLookup's generator (rsx_dng_post_core.h), the idea of
tests/test_dither_jump_model.py carried to seeds that are NOT below the modulus.

v' = 15700 (v & 65535) + (v >> 16) multiplies by 15700 modulo m = 15700 * 2^16 - 1.  doLookup's
row seed (dim_x + 13 y) ^ 0x45694584 lies between m and 2 m, and it steps before it uses: sample x
sees the state x + 1 steps behind the seed.  What the core relies on:
  * the state n >= 2 steps behind the seed equals ((seed mod m) 15700^n) mod m;
  * after ONE step that holds too, except for seeds whose low half is 65535 -- there the state is
    not below m (so the lane that owns sample 0 steps the seed itself);
  * no seed of this kind is congruent to 0 mod m (the fixed points 0 and m are never reached).
The first three tests are that argument in numbers: plain arithmetic, true with or without the
library.  The fourth holds the host build's rsx_dng_post_host_dither_state() -- the lanes' arithmetic
-- against the plain loop, on rows that include the exceptional ones."""
import ctypes as C

import numpy as np
import pytest

import dng_post_files as K
from rawspeed_amd import build

M = 15700 * 65536 - 1
A = 15700


def step(v):
    return (A * (v & 65535) + (v >> 16)) & 0xFFFFFFFF


def seed(dim_x, y):
    return (dim_x + 13 * y) ^ 0x45694584


def test_seeds_lie_between_m_and_2m_and_are_not_multiples_of_m():
    t = np.arange(1, 1 << 20, dtype=np.int64)  # dim_x + 13 y: what validate() admits
    s = t ^ 0x45694584
    assert (s > M).all() and (s < 2 * M).all()
    assert ((s >> 16) >= 0x4560).all() and ((s >> 16) <= 0x456F).all()
    assert (s % M != 0).all()


def test_one_step_leaves_a_residue_unless_the_low_half_is_ffff():
    t = np.arange(1, 1 << 20, dtype=np.int64)
    s = t ^ 0x45694584
    one = A * (s & 65535) + (s >> 16)
    want = (s % M) * A % M
    special = (s & 65535) == 65535
    assert special.sum() == 16 and ((t[special] & 0xFFFF) == 0xBA7B).all()
    assert (one[~special] == want[~special]).all()
    assert (one[special] >= M).all() and (one[special] % M == want[special]).all()
    two = A * (one & 65535) + (one >> 16)
    assert (two == want * A % M).all() and (two < M).all()


def test_the_states_equal_the_powers_from_two_steps_on():
    rng = np.random.default_rng(0xD17)
    sums = np.concatenate([rng.integers(1, 1 << 20, size=300), [0xBA7B, 0x1BA7B, 0xFBA7B, 1, (1 << 20) - 1]])
    for t in sums:
        s = int(t) ^ 0x45694584
        v, p = s, s % M
        for n in range(1, 400):
            v, p = step(v), p * A % M
            if n >= 2:
                assert v == p, (t, n)


@pytest.fixture(scope="module")
def host():
    lib_path, _ = build.build_dng_post_host()
    L = C.CDLL(lib_path)
    L.rsx_dng_post_host_dither_state.argtypes = [C.c_uint32] * 3
    L.rsx_dng_post_host_dither_state.restype = C.c_uint32
    return L


def test_the_lanes_jump_matches_the_plain_loop(host):
    rng = np.random.default_rng(0xD18)
    rows = [(7998, 3057), (70000, 2), (64, 0), (0xBA7B, 0), (6000, 4000)] + \
        [(int(rng.integers(1, 70000)), int(rng.integers(0, 9000))) for _ in range(10)]
    for dim_x, y in rows:
        n = min(dim_x * 3, 70000 if dim_x == 70000 else 9000)
        states = K.dither_states(dim_x, [y], n)[0]
        xs = np.unique(np.concatenate([np.arange(0, 40), rng.integers(0, n, size=60), [n - 1]]))
        for x in xs[xs < n]:
            assert host.rsx_dng_post_host_dither_state(dim_x, y, int(x)) == int(states[x]), (dim_x, y, x)
    assert seed(7998, 3057) & 65535 == 65535

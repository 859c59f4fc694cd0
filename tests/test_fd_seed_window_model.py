"""Exact integer model of the two-level seeding of the forward-difference X path (fdplan::plan in host_fd_plan.h, k_modp_fd_table and
k_modp_fd_step in modp_kernels.hip) over a small safe prime: Horner's rule at the t MIDDLE positions of the seed window, the
difference table of those t values, and the stride-1 chain stepping forward and backward from them to the window's ends.

The model follows the host's index arithmetic (S, chain_len, w0, seed0, m0, w1, steps per direction) and the kernels' rules
(state / state_back diagonals of the table, H_l *= H_{l+1} per step, the `step >= t` store rule, j = w0 + step forward and
j = w0 + t - 1 - step backward) and checks what the launch must guarantee whatever the group is: every seed position outside
the Horner window written exactly once, nothing outside [0, m0), the values those of direct evaluation, and
max(m0 - 1 - w1, w1 + t - 1) serial steps."""
import random

import pytest

P = 2879                      # safe prime: (P - 1) / 2 = 1439 is prime
ORDER = P - 1                 # the commitments' exponents live mod P - 1, as the reference's do mod q - 1


def host_plan(t, n, busy=True):
    """S, chain_len, w0, seed0, m0, w1 as the X path's plan has them (fdplan::plan in mpvss_rs_amd/csrc/host_fd_plan.h, which
    tests/test_fd_plan_host.py holds to this transcription; 16 chains for t <= 256: a call that has the GPU to itself, and a box
    among others from 65536 shares)"""
    S = max(max(min(2048 // t, n // 8192), n // 16384), 4)
    if (not busy or n >= 65536) and t <= 256:
        S = max(S, 16)
    S = max(1, min(S, n // (4 * t)))
    chain_len = (n + S - 1) // S
    w0 = (chain_len - t) // 2
    seed0 = S * w0
    m0 = S * t
    w1 = (m0 - t) // 2
    return S, chain_len, w0, seed0, m0, w1


def evaluate(cm, pos):
    """X = prod C_j^(pos^j) mod P: the commitment multi-exponentiation, directly"""
    x, e = 1, 1
    for c in cm:
        x = x * pow(c, e, P) % P
        e = e * pos % ORDER
    return x


def difference_table(x):
    """k_modp_fd_table for one chain: E_l[k] = E_{l-1}[k+1] F_{l-1}[k], F_l[k] = F_{l-1}[k+1] E_{l-1}[k] with F = E^-1;
    state[l] = E_l[0] (forward), state_back[l] = (l even ? E_l : F_l)[t-1-l] (backward)"""
    t = len(x)
    E = list(x)
    F = [pow(v, -1, P) for v in x]
    state, back = [E[0]], [E[t - 1]]
    for lvl in range(1, t):
        E, F = ([E[k + 1] * F[k] % P for k in range(t - lvl)], [F[k + 1] * E[k] % P for k in range(t - lvl)])
        state.append(E[0])
        back.append((F if lvl & 1 else E)[t - 1 - lvl])
    return state, back


def step_chain(table, t, w0, chain_len, count, direction, x_m, writes, chains=1, chain=0):
    """k_modp_fd_step for one chain and direction: every level times the level below it, once per step (lock step: the old value
    of the level below); the bottom stage stores from step t on.  Returns the number of serial steps."""
    if direction == 1 and w0 == 0:
        return 0
    steps = chain_len - 1 - w0 if direction == 0 else w0 + t - 1
    D = list(table)
    for step in range(1, steps + 1):
        D = [D[k] * (D[k + 1] if k + 1 < t else 1) % P for k in range(t)]
        j = w0 + step if direction == 0 else w0 + t - 1 - step
        idx = chain + chains * j
        if step >= t and idx < count:
            assert 0 <= idx, (direction, step, j)
            x_m[idx] = D[0]
            writes[idx] = writes.get(idx, 0) + 1
    return steps


CASES = [(t, n) for t in (16, 17, 33, 64) for n in (16 * t, 16 * t + 1, 20 * t + 3, 4096, 5000)]


@pytest.mark.parametrize("t,n", CASES)
def test_seed_window_stepped_both_ways_from_its_middle(t, n):
    rng = random.Random(t * 100003 + n)
    cm = [pow(4, rng.randrange(1, ORDER), P) for _ in range(t)]
    first = rng.choice((1, 777, 1 << 40))
    S, chain_len, w0, seed0, m0, w1 = host_plan(t, n)
    assert S >= 4 and seed0 + m0 <= n and 0 <= w1 and w1 + t <= m0
    direct = [evaluate(cm, first + seed0 + i) for i in range(m0)]
    # level 1: Horner at w1 .. w1 + t - 1 of the seed window, into xseed + w1
    xseed = {w1 + k: direct[w1 + k] for k in range(t)}
    state, back = difference_table([xseed[w1 + k] for k in range(t)])
    writes = {}
    fwd = step_chain(state, t, w1, m0, m0, 0, xseed, writes)
    bwd = step_chain(back, t, w1, m0, m0, 1, xseed, writes)
    assert max(fwd, bwd) == max(m0 - 1 - w1, w1 + t - 1)
    assert (bwd == 0) == (w1 == 0)
    assert all(0 <= i < m0 for i in writes), "a store outside the seed window"
    outside = [i for i in range(m0) if not w1 <= i < w1 + t]
    assert sorted(writes) == outside and all(writes[i] == 1 for i in outside)
    assert [xseed[i] for i in range(m0)] == direct
    # level 2: the S strided chains from the seed window in their middle reach every position of the box exactly once
    x_m = {seed0 + i: v for i, v in xseed.items()}
    writes2 = {}
    for c in range(S):
        st2, bk2 = difference_table([x_m[c + S * (w0 + k)] for k in range(t)])
        f2 = step_chain(st2, t, w0, chain_len, n, 0, x_m, writes2, S, c)
        b2 = step_chain(bk2, t, w0, chain_len, n, 1, x_m, writes2, S, c)
        assert f2 == chain_len - 1 - w0 and b2 == (w0 + t - 1 if w0 else 0)
    rest = [i for i in range(n) if not seed0 <= i < seed0 + m0]
    assert sorted(writes2) == rest and all(writes2[i] == 1 for i in rest)
    for i in rng.sample(range(n), 24) + [0, n - 1]:
        assert x_m[i] == evaluate(cm, first + i), i


def test_a_window_of_t_positions_steps_forward_only():
    """w1 == 0 (m0 == t, one chain): no backward pipeline, as before"""
    t = 16
    cm = [pow(4, 3 + 5 * j, P) for j in range(t)]
    x = {k: evaluate(cm, 1 + k) for k in range(t)}
    state, back = difference_table([x[k] for k in range(t)])
    writes = {}
    assert step_chain(back, t, 0, t, t, 1, x, writes) == 0 and step_chain(state, t, 0, t, t, 0, x, writes) == t - 1 and not writes


def test_headline_step_counts():
    """(65536, 256): 16 chains, 2 175 serial steps at either level (one-way seeding would take 4 095 at the first); the 8 chains of
    before: 1 151 instead of 2 047 first-level steps, 4 223 at the second"""
    S, chain_len, w0, seed0, m0, w1 = host_plan(256, 65536)
    assert (S, m0, w1) == (16, 4096, 1920) and max(m0 - 1 - w1, w1 + 255) == 2175 and chain_len - 1 - w0 == 2175
    assert host_plan(256, 65536, busy=False)[0] == 16 and host_plan(256, 32768)[0] == 4 and host_plan(512, 65536)[0] == 4
    m0, w1 = 8 * 256, (8 * 256 - 256) // 2
    assert max(m0 - 1 - w1, w1 + 255) == 1151 and (65536 // 8) - 1 - (65536 // 8 - 256) // 2 == 4223

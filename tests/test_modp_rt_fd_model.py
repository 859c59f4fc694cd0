"""Integer model of the forward differences of a run-time MODP group (k_rt_fd_chain, rt_commit_eval_dev).

The model follows the kernels step by step -- seeds and inverse seeds by Horner over the commitments and the inverted
commitments, the table E_l[k] = E_{l-1}[k+1] F_{l-1}[k], F_l[k] = F_{l-1}[k+1] E_{l-1}[k] with both of its diagonals, the
in-place form of it that the kernel runs (one level per quad, the backward direction as the forward rule over the reversed
seeds), and the lock-step stepping D_k <- D_k D_{k+1} in both directions -- and counts every product.  X must equal
prod_j C_j^(i^j) computed with pow; the mutants at the end show that each rule the kernel depends on is pinned."""
import random

import pytest

Q = 2 ** 127 - 1          # any odd modulus serves: the identities are integer identities in the exponent
Q_SMALL = 1019            # a safe prime whose q - 1 the positions can reach


class Count:
    def __init__(self):
        self.products = self.horner = self.table = self.steps = 0


def chain_bounds(n, S, c):
    """modp_rt_fd_chain"""
    a, b = c * n // S, (c + 1) * n // S
    return a, b - a


def reference(C, q, positions):
    out = []
    for i in positions:
        x = 1
        for j, cj in enumerate(C):
            x = x * pow(cj, i ** j, q) % q
        out.append(x)
    return out


def horner(C, q, i, cnt):
    """X(i) by Horner's rule in the exponent, as k_rt_commit_eval: one evaluation"""
    cnt.horner += 1
    acc = C[-1]
    for cj in reversed(C[:-1]):
        acc = pow(acc, i, q) * cj % q
    return acc


def invert_all(C, q):
    """Montgomery's trick: one inversion and 3 (t - 1) products"""
    pre, prods = [C[0] % q], 0
    for c in C[1:]:
        pre.append(pre[-1] * c % q)
        prods += 1
    run = pow(pre[-1], -1, q)
    inv = [0] * len(C)
    for j in range(len(C) - 1, 0, -1):
        inv[j] = run * pre[j - 1] % q
        run = run * C[j] % q
        prods += 2
    inv[0] = run
    return inv, prods


def table(E0, F0, q, cnt, swap_at=None):
    """the triangular table of the scheme; returns the forward state D_l = E_l[0] and the backward state
    B_l = E_l[t-1-l] (l even), F_l[t-1-l] (l odd)"""
    t = len(E0)
    E, F = list(E0), list(F0)
    fwd, bwd = [E[0]], [E[t - 1]]
    for l in range(1, t):
        if swap_at == l:      # mutant: roles of E and F swapped in this step
            En = [F[k + 1] * E[k] % q for k in range(t - l)]
            Fn = [E[k + 1] * F[k] % q for k in range(t - l)]
        else:
            En = [E[k + 1] * F[k] % q for k in range(t - l)]
            Fn = [F[k + 1] * E[k] % q for k in range(t - l)]
        cnt.table += 2 * (t - l)
        E, F = En, Fn
        fwd.append(E[0])
        bwd.append(E[t - 1 - l] if l % 2 == 0 else F[t - 1 - l])
    return fwd, bwd


def table_in_place(G0, H0, q):
    """what k_rt_fd_chain runs: level l updates the quads k >= l from their lower neighbour; quad k ends with D_k"""
    t = len(G0)
    G, H = list(G0), list(H0)
    for l in range(1, t):
        Gn, Hn = list(G), list(H)
        for k in range(l, t):
            Gn[k] = G[k] * H[k - 1] % q
            Hn[k] = H[k] * G[k - 1] % q
        G, H = Gn, Hn
    return G


def step(D, q, cnt, stale=True):
    """one lock-step step: every level multiplies by the copy of D_{k+1} stored BEFORE the step"""
    t = len(D)
    if stale:
        new = [D[k] * D[k + 1] % q for k in range(t - 1)] + [D[t - 1]]
    else:                     # mutant: levels run from the top down and read the already updated neighbour
        new = list(D)
        for k in range(t - 2, -1, -1):
            new[k] = new[k] * new[k + 1] % q
    cnt.steps += 1
    cnt.products += t - 1
    return new


def fd_eval(C, q, p0, n, S, swap_at=None, wrong_parity=False, stale=True, in_place=False):
    """X at p0 .. p0+n-1 through S chains, and the counts"""
    t = len(C)
    cnt = Count()
    Cinv, inv_products = invert_all(C, q)
    X = [None] * n
    for c in range(S):
        first, length = chain_bounds(n, S, c)
        assert length >= t
        s0 = first + (length - t) // 2
        E0 = [horner(C, q, p0 + s0 + k, cnt) for k in range(t)]
        F0 = [horner(Cinv, q, p0 + s0 + k, cnt) for k in range(t)]
        for k in range(t):
            X[s0 + k] = E0[k]
        if in_place:
            fwd = table_in_place(E0, F0, q)
            bwd = table_in_place(E0[::-1], F0[::-1], q)
        else:
            fwd, bwd = table(E0, F0, q, cnt, swap_at)
            if wrong_parity:
                _, other = table(F0, E0, q, Count())       # the other diagonal: parities exchanged
                bwd = other
        D = fwd
        m = first + length - (s0 + t)
        for i in range(1, (t - 1 + m if m > 0 else 0) + 1):
            D = step(D, q, cnt, stale)
            if i >= t:
                X[s0 + i] = D[0]
        D = bwd
        m = s0 - first
        for i in range(1, (t - 1 + m if m > 0 else 0) + 1):
            D = step(D, q, cnt, stale)
            if i >= t:
                X[s0 + t - 1 - i] = D[0]
    return X, cnt, inv_products


def commitments(t, q, seed):
    rng = random.Random(seed)
    return [rng.randrange(2, q) for _ in range(t)]


CASES = [(t, S, n, p0)
         for t in (2, 3, 16, 17)
         for S, n in ((1, t), (1, 2 * t + 5), (2, 4 * t + 3), (3, 3 * t + 2), (3, 7 * t + 1))
         for p0 in (0, 1, 2 ** 40)]


@pytest.mark.parametrize("t,S,n,p0", CASES)
def test_parity_with_pow(t, S, n, p0):
    C = commitments(t, Q, 100 * t + S)
    want = reference(C, Q, range(p0, p0 + n))
    got, _, _ = fd_eval(C, Q, p0, n, S)
    assert got == want
    got2, _, _ = fd_eval(C, Q, p0, n, S, in_place=True)
    assert got2 == want, "the kernel's in-place table differs from the scheme's"


def test_ragged_chains_cover_every_position_once():
    for n, S in ((50, 3), (100, 7), (17, 1), (65536, 32)):
        spans = [chain_bounds(n, S, c) for c in range(S)]
        assert spans[0][0] == 0 and sum(l for _, l in spans) == n
        for (a, l), (b, _) in zip(spans, spans[1:]):
            assert a + l == b
        assert min(l for _, l in spans) >= n // S


@pytest.mark.parametrize("t,S,n", [(2, 1, 9), (3, 2, 40), (16, 3, 200), (17, 2, 120)])
def test_counts(t, S, n):
    C = commitments(t, Q, t)
    _, cnt, inv_products = fd_eval(C, Q, 5, n, S)
    assert inv_products == 3 * (t - 1)
    assert cnt.horner == S * 2 * t                           # set-up per chain: 2 t Horner evaluations ...
    assert cnt.table == S * 2 * (t * (t - 1) // 2)           # ... plus the table
    assert cnt.products == cnt.steps * (t - 1)               # t - 1 products per stepped share
    want = 0                                                 # a direction with m > 0 shares first walks over the t - 1 other seeds
    for c in range(S):
        first, length = chain_bounds(n, S, c)
        s0 = first + (length - t) // 2
        for m in (first + length - (s0 + t), s0 - first):
            want += t - 1 + m if m > 0 else 0
    assert cnt.steps == want


# ---- the host gate (rt_fd_prepare, rt_fd_positions_ok, rt_commit_eval_dev) -------------------------------------------------
def admissible(q, C, positions, t_max, min_shares, mode):
    import math
    t, n = len(C), len(positions)
    if mode == 0:
        return False
    if not 2 <= t <= t_max:
        return False
    if n < t or (mode == 1 and n < min_shares):
        return False
    if any(math.gcd(c % q, q) != 1 for c in C):
        return False
    p0 = positions[0]
    if p0 < 0 or any(p != p0 + i for i, p in enumerate(positions)):
        return False
    if q - 1 < 2 ** 64 and p0 + n - 1 >= q - 1:
        return False
    return True


def test_host_gate_clause_by_clause():
    q, t = Q_SMALL, 4
    C = commitments(t, q, 1)
    ok = dict(q=q, C=C, positions=list(range(3, 43)), t_max=256, min_shares=32, mode=1)
    assert admissible(**ok)
    assert not admissible(**{**ok, "mode": 0})
    assert not admissible(**{**ok, "positions": [3, 4, 6] + list(range(7, 44))})          # not consecutive
    assert not admissible(**{**ok, "positions": list(range(-1, 39))})                     # p0 < 0
    assert not admissible(**{**ok, "positions": list(range(q - 5, q + 35))})              # reaches q - 1
    assert admissible(**{**ok, "positions": list(range(q - 41, q - 1))})                  # last position q - 2
    assert not admissible(**{**ok, "C": C[:2] + [0] + C[3:]})                             # a commitment 0 mod q
    assert not admissible(**{**ok, "C": C[:2] + [q] + C[3:]})
    assert not admissible(**{**ok, "q": 1015, "C": [5, 2, 3, 4]})                         # 5 divides 1015: no unit
    assert not admissible(**{**ok, "C": C[:1]})                                           # t = 1
    assert not admissible(**{**ok, "t_max": 3})                                           # t above t_max
    assert not admissible(**{**ok, "min_shares": 41})                                     # below min_shares in mode 1 ...
    assert admissible(**{**ok, "min_shares": 41, "mode": 2})                              # ... which mode 2 ignores
    assert not admissible(**{**ok, "positions": [3, 4, 5], "mode": 2})                    # fewer positions than seeds
    got, _, _ = fd_eval(C, q, q - 41, 40, 2)
    assert got == reference(C, q, range(q - 41, q - 1))


def test_composite_modulus_units_only():
    q = 1015 * 1019                      # odd, composite
    C = [2, 3, 1019 + 2, 8]
    got, _, _ = fd_eval(C, q, 7, 30, 2)
    assert got == reference(C, q, range(7, 37))


# ---- mutants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [3, 16, 17])
def test_mutants_are_caught(t):
    C = commitments(t, Q, 7 * t)
    n, S, p0 = 4 * t + 3, 2, 1
    want = reference(C, Q, range(p0, p0 + n))
    assert fd_eval(C, Q, p0, n, S)[0] == want
    assert fd_eval(C, Q, p0, n, S, swap_at=1)[0] != want, "E/F roles swapped in a table step"
    assert fd_eval(C, Q, p0, n, S, swap_at=t - 1)[0] != want
    assert fd_eval(C, Q, p0, n, S, wrong_parity=True)[0] != want, "backward state from the wrong diagonal parity"
    assert fd_eval(C, Q, p0, n, S, stale=False)[0] != want, "a step that reads an already updated D_{k+1}"

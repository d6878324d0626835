"""ss_edit_distance / ss_nbest_risk (csrc/edit_distance.hip) and the scoring surface of recognition_model against tests/edit_distance_oracle.py.
Everything is an integer, or an f64 sum in a fixed order: every comparison is exact equality."""
import ctypes
import random

import numpy as np
import pytest
import torch

from silent_speech_amd import _lib, asr_evaluation
from silent_speech_amd import recognition_model as rm
from silent_speech_amd import torch_ops  # noqa: F401
from tests import edit_distance_oracle as oracle
from tests.backend import dev, is_emu  # noqa: F401

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _layout(seqs, gap=0, fill=0, seed=0):
    """flat tokens (gap entries of garbage before every sequence and behind the last) and the (first, length) table"""
    rng = np.random.RandomState(seed)
    flat, rows = [], []
    for s in seqs:
        flat.extend(rng.randint(-5, 60, gap).tolist() if fill is None else [fill] * gap)
        rows.append((len(flat), len(s)))
        flat.extend(int(x) for x in s)
    flat.extend(rng.randint(-5, 60, gap + 1).tolist() if fill is None else [fill] * (gap + 1))
    return np.asarray(flat, dtype=np.int32), np.asarray(rows, dtype=np.int64).reshape(len(rows), 2)


def _run(dev, flat, rows, pairs, want_ops=True):
    """The op on host tables -> (dist, counts, [ops bytes of every pair, to its capacity])"""
    t, s = torch.from_numpy(np.ascontiguousarray(flat)).to(dev), torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    p = torch.from_numpy(np.asarray(pairs, dtype=np.int32).reshape(len(pairs), 2)).to(dev)
    dist, counts, ops, first = torch.ops.silent_speech.edit_distance(t, s, p, want_ops)
    dist, counts, ops, first = dist.cpu().numpy(), counts.cpu().numpy(), ops.cpu().numpy(), first.cpu().numpy()
    assert dist.shape == (len(pairs),) and counts.shape == (len(pairs), 4)
    if not want_ops:
        assert ops.size == 0 and first.size == 0
        return dist, counts, None
    assert first.shape == (len(pairs) + 1,) and first[0] == 0 and first[-1] == ops.size
    return dist, counts, [ops[first[k]:first[k + 1]] for k in range(len(pairs))]


def _check(seqs, pairs, got, want=None):
    dist, counts, ops = got
    for k, (ia, ib) in enumerate(pairs):
        d, c, o = want[k] if want is not None else oracle.align(seqs[ia], seqs[ib])
        assert dist[k] == d and tuple(counts[k]) == c, (k, len(seqs[ia]), len(seqs[ib]))
        if ops is not None:
            assert ops[k].size == len(seqs[ia]) + len(seqs[ib])
            assert np.array_equal(ops[k][:o.size], o), (k, len(seqs[ia]), len(seqs[ib]))
            assert (ops[k][o.size:] == -1).all()


# ------------------------------------------------------------------------------------------------ 1. the oracle itself
def test_oracle_against_an_independent_recursion_and_its_identities():
    rng = random.Random(0)
    for _ in range(2000):
        sym = rng.randint(1, 3)
        a = [rng.randrange(sym) for _ in range(rng.randint(0, 8))]
        b = [rng.randrange(sym) for _ in range(rng.randint(0, 8))]
        d, (h, s, de, i), ops = oracle.align(a, b)
        assert d == oracle.distance_recursive(a, b) == oracle.distance(b, a)
        assert h + s + de == len(a) and h + s + i == len(b) and s + de + i == d
        out = oracle.replay(a, ops)
        assert len(out) == len(b) and all(x is None or x == y for x, y in zip(out, b))
        # the steps that are not hits really change something: a substitution never sits on equal tokens
        ia = ib = 0
        for op in ops:
            if op == oracle.SUB:
                assert a[ia] != b[ib]
            ia += op in (oracle.HIT, oracle.SUB, oracle.DEL)
            ib += op in (oracle.HIT, oracle.SUB, oracle.INS)


# ------------------------------------------------------------------------------------------------ 2. the tie rule
TIE_CASES = [
    ([1, 2], [2, 1], 2, (0, 2, 0, 0), [1, 1]),                           # two substitutions, not a deletion and an insertion
    ([3, 3, 3, 3], [3, 3, 3, 3], 0, (4, 0, 0, 0), [0, 0, 0, 0]),
    ([1, 2, 3], [4, 5, 6], 3, (0, 3, 0, 0), [1, 1, 1]),
    ([1, 2, 3], [], 3, (0, 0, 3, 0), [2, 2, 2]),
    ([], [7, 8], 2, (0, 0, 0, 2), [3, 3]),
    ([], [], 0, (0, 0, 0, 0), []),
    ([5, 5, 5], [5], 2, (1, 0, 2, 0), [2, 2, 0]),                        # the hit sits on the LAST of the repeated tokens (diagonal first from the end)
    ([5], [5, 5, 5], 2, (1, 0, 0, 2), [3, 3, 0]),
    ([1, 5, 5, 2], [5], 3, (1, 0, 3, 0), None),
    ([1, 2, 1, 2, 1], [2, 1, 2], 2, (3, 0, 2, 0), None),
]


def test_tie_rule_on_constructed_cases(dev):
    seqs, pairs = [], []
    for a, b, _, _, _ in TIE_CASES:
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [a, b]
    for a, b, d, c, o in TIE_CASES:                                       # what the oracle says is what the case was constructed for
        od, oc, oo = oracle.align(a, b)
        assert (od, oc) == (d, c) and (o is None or oo.tolist() == o)
    flat, rows = _layout(seqs)
    _check(seqs, pairs, _run(dev, flat, rows, pairs))
    _check(seqs, pairs, _run(dev, flat, rows, pairs, want_ops=False))


# ------------------------------------------------------------------------------------------------ 3. instance and lane edges
NB = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023]
NA = [0, 1, 64, 65, 1023]


def _edge_case(symbols):
    rng = np.random.RandomState(symbols)
    seqs = [rng.randint(0, symbols, n).tolist() for n in NA] + [rng.randint(0, symbols, n).tolist() for n in NB]
    pairs = [(i, len(NA) + j) for i in range(len(NA)) for j in range(len(NB))]
    if symbols == 2:
        pairs.append((len(NA) - 1, len(seqs) - 1))                       # (repeated: the grid has 1023 x 1023 already; kept as the issue lists it)
    return seqs, pairs, [oracle.align(seqs[a], seqs[b]) for a, b in pairs]


@pytest.mark.parametrize('symbols', [2, 50])
def test_instance_and_lane_edges(dev, symbols):
    seqs, pairs, want = _once(('edges', symbols), lambda: _edge_case(symbols))
    flat, rows = _layout(seqs)
    _check(seqs, pairs, _run(dev, flat, rows, pairs), want)
    got = _run(dev, flat, rows, pairs, want_ops=False)                    # the count-only instance of every lane width
    _check(seqs, pairs, got, want)


def test_long_equal_and_shifted_strings(dev):
    """1023 x 1023 once more where the path is known: a string against itself, and against itself shifted by one."""
    rng = np.random.RandomState(7)
    a = rng.randint(0, 1000, 1023).tolist()
    seqs = [a, list(a), a[1:] + [1001]]
    pairs = [(0, 1), (0, 2), (2, 0)]
    want = _once('shifted', lambda: [oracle.align(seqs[x], seqs[y]) for x, y in pairs])
    assert want[0][0] == 0 and want[1][0] == 2
    flat, rows = _layout(seqs)
    _check(seqs, pairs, _run(dev, flat, rows, pairs), want)


# ------------------------------------------------------------------------------------------------ 4. isolation
def _isolation_case():
    rng = np.random.RandomState(11)
    seqs = [rng.randint(0, 4, n).tolist() for n in (0, 3, 17, 64, 65, 70, 130, 150, 9, 1, 129, 40)]
    pairs = [(0, 1), (1, 0), (2, 3), (3, 4), (5, 6), (6, 7), (7, 5), (8, 9), (10, 6), (11, 11), (4, 10), (2, 2)]
    return seqs, pairs, [oracle.align(seqs[a], seqs[b]) for a, b in pairs]


def test_pairs_do_not_see_each_other(dev):
    seqs, pairs, want = _once('isolation', _isolation_case)
    flat, rows = _layout(seqs)
    base = _run(dev, flat, rows, pairs)
    _check(seqs, pairs, base, want)

    def same(got, order):
        for k, src in enumerate(order):
            assert got[0][k] == base[0][src] and np.array_equal(got[1][k], base[1][src]) and np.array_equal(got[2][k], base[2][src])
    for seed in (1, 2):                                                   # gaps between the sequences, different garbage in them
        f2, r2 = _layout(seqs, gap=5, fill=None, seed=seed)
        same(_run(dev, f2, r2, pairs), range(len(pairs)))
    perm = np.random.RandomState(3).permutation(len(pairs)).tolist()     # permuted
    same(_run(dev, flat, rows, [pairs[k] for k in perm]), perm)
    extra = [[1, 2, 3] * 30, [3, 2, 1] * 50]                              # unrelated pairs added, before and behind
    f3, r3 = _layout(extra + seqs, gap=2, fill=-7)
    shifted = [(a + 2, b + 2) for a, b in pairs]
    got = _run(dev, f3, r3, [(0, 1)] + shifted + [(1, 0), (0, 0)])
    same((got[0][1:], got[1][1:], got[2][1:]), range(len(pairs)))


def test_nothing_is_written_outside_a_pairs_bytes(dev):
    """The C entry point with guard bytes before, between and behind the pairs' ops bytes, and more room than n_a + n_b for some pairs."""
    seqs, pairs, want = _once('isolation', _isolation_case)
    flat, rows = _layout(seqs, gap=3, fill=None, seed=5)
    G = 37
    first, at = [], G
    for k, (a, b) in enumerate(pairs):
        first.append(at)
        at += len(seqs[a]) + len(seqs[b]) + (k % 3)                        # 0 .. 2 spare bytes: filled with -1 as well
    first.append(at)
    n_ops = at + G
    L = _lib.lib()
    t, s = torch.from_numpy(flat).to(dev), torch.from_numpy(rows).to(dev)
    p = torch.tensor(pairs, dtype=torch.int32).to(dev)
    f = torch.tensor(first, dtype=torch.int64).to(dev)
    ops = torch.full((n_ops,), 0x55, dtype=torch.int8).to(dev)
    dist = torch.full((len(pairs) + 2,), 77, dtype=torch.int32).to(dev)
    counts = torch.full((len(pairs) + 2, 4), 77, dtype=torch.int32).to(dev)
    ws_bytes = L.ss_edit_distance_workspace_bytes(len(pairs), n_ops)
    assert ws_bytes == 256 * (n_ops + 64 * len(pairs))
    ws = torch.full((ws_bytes // 4 + 64,), 0x5A5A5A5A, dtype=torch.int32).to(dev)
    _lib.check(L.ss_edit_distance(_lib.ptr(t), t.shape[0], _lib.ptr(s), s.shape[0], _lib.ptr(p), len(pairs), ctypes.c_void_p(dist.data_ptr() + 4),
                                  ctypes.c_void_p(counts.data_ptr() + 16), _lib.ptr(ops), _lib.ptr(f), n_ops, _lib.ptr(ws), _lib.stream_of(t)))
    ops, dist, counts, ws = ops.cpu().numpy(), dist.cpu().numpy(), counts.cpu().numpy(), ws.cpu().numpy()
    assert (ops[:G] == 0x55).all() and (ops[at:] == 0x55).all()
    assert dist[0] == 77 and dist[-1] == 77 and (counts[0] == 77).all() and (counts[-1] == 77).all()
    assert (ws[ws_bytes // 4:] == 0x5A5A5A5A).all()
    for k, (d, c, o) in enumerate(want):
        region = ops[first[k]:first[k + 1]]
        assert dist[1 + k] == d and tuple(counts[1 + k]) == c
        assert np.array_equal(region[:o.size], o) and (region[o.size:] == -1).all()
    assert L.ss_edit_distance_workspace_bytes(-1, 0) == -1 and L.ss_edit_distance_workspace_bytes(1, -1) == -1


def test_no_pairs_launch_nothing(dev):
    flat, rows = _layout([[1, 2]])
    dist, counts, ops = _run(dev, flat, rows, [])
    assert dist.size == 0 and counts.size == 0 and ops == []


# ------------------------------------------------------------------------------------------------ 5. bad tables
def test_bad_table_entries_are_cut_short(dev):
    seqs = [[1, 2, 3, 4], [1, 3, 4], [2] * 70, [2, 1] * 40]
    flat, rows = _layout(seqs)
    n_tok = flat.shape[0]
    bad_rows = np.concatenate([rows, np.asarray([(0, -1), (0, 1024), (n_tok - 2, 3), (-1, 2), (n_tok, 1)], dtype=np.int64)])
    NEG, LONG, PAST, BEFORE, BEHIND = range(4, 9)
    pairs = [(0, 1), (NEG, 1), (2, 3), (0, LONG), (PAST, 0), (1, 0), (0, 9), (-1, 0), (3, BEFORE), (BEHIND, BEHIND), (3, 2), (0, 2 ** 31 - 1)]
    good = [k for k, (a, b) in enumerate(pairs) if 0 <= a < 4 and 0 <= b < 4]
    assert len(good) == 4
    for want_ops in (True, False):
        dist, counts, ops = _run(dev, flat, bad_rows, pairs, want_ops)
        for k, (a, b) in enumerate(pairs):
            if k in good:
                d, c, o = oracle.align(seqs[a], seqs[b])
                assert dist[k] == d and tuple(counts[k]) == c
                if want_ops:
                    assert np.array_equal(ops[k][:o.size], o) and (ops[k][o.size:] == -1).all() and ops[k].size == len(seqs[a]) + len(seqs[b])
            else:
                assert dist[k] == -1 and (counts[k] == -1).all()
                if want_ops:
                    assert (ops[k] == -1).all()


def test_bad_ops_table_entries(dev):
    """Through the C entry point: bytes that leave ops, too few bytes, a decreasing table -> that pair -1 (and -1 in the bytes it does own)."""
    seqs = [[1, 2, 3, 4], [1, 3, 4], [4, 4]]
    flat, rows = _layout(seqs)
    pairs = [(0, 1), (0, 2), (1, 2), (2, 0), (0, 1)]
    first = [0, 7, 12, 200, 190, 197]                                    # pair 1: 5 < 6 bytes; pair 2: leaves ops; pair 3: decreasing; pair 4: fine
    n_ops = 197
    L = _lib.lib()
    t, s = torch.from_numpy(flat).to(dev), torch.from_numpy(rows).to(dev)
    p, f = torch.tensor(pairs, dtype=torch.int32).to(dev), torch.tensor(first, dtype=torch.int64).to(dev)
    ops = torch.full((n_ops + 16,), 0x55, dtype=torch.int8).to(dev)
    dist = torch.full((5,), 77, dtype=torch.int32).to(dev)
    counts = torch.full((5, 4), 77, dtype=torch.int32).to(dev)
    ws = torch.zeros(L.ss_edit_distance_workspace_bytes(5, n_ops) // 4, dtype=torch.int32).to(dev)
    _lib.check(L.ss_edit_distance(_lib.ptr(t), t.shape[0], _lib.ptr(s), s.shape[0], _lib.ptr(p), 5, _lib.ptr(dist), _lib.ptr(counts), _lib.ptr(ops),
                                  _lib.ptr(f), n_ops, _lib.ptr(ws), _lib.stream_of(t)))
    ops, dist = ops.cpu().numpy(), dist.cpu().numpy()
    d0, _, o0 = oracle.align(seqs[0], seqs[1])
    assert dist.tolist() == [d0, -1, -1, -1, d0]
    assert np.array_equal(ops[:o0.size], o0) and (ops[o0.size:7] == -1).all() and (ops[7:12] == -1).all()
    assert (ops[12:190] == 0x55).all() and np.array_equal(ops[190:190 + o0.size], o0) and (ops[190 + o0.size:197] == -1).all()
    assert (ops[197:] == 0x55).all()


def test_python_side_arguments_raise_before_any_launch(dev):
    t = torch.zeros(4, dtype=torch.int32, device=dev)
    s = torch.tensor([[0, 2], [2, 2]], dtype=torch.int64, device=dev)
    p = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    w = torch.tensor([0.5, 0.5], dtype=torch.float32, device=dev)
    ed, nr = torch.ops.silent_speech.edit_distance, torch.ops.silent_speech.nbest_risk
    for args in [(t.to(torch.int64), s, p), (t, s.to(torch.int32), p), (t, s, p.to(torch.int64)), (t, s.reshape(-1), p), (t, s, p.reshape(-1)),
                 (t, s, torch.zeros((1, 3), dtype=torch.int32, device=dev))]:
        with pytest.raises(RuntimeError):
            ed(*args, False)
    g = torch.tensor([[0, 2]], dtype=torch.int64, device=dev)
    for args in [(t, s, g.to(torch.int32), w), (t, s, g, w.to(torch.float64)), (t, s, g, w[:1]), (t, s, torch.tensor([[0, 0]], dtype=torch.int64, device=dev), w),
                 (t, s, torch.tensor([[0, 129]], dtype=torch.int64, device=dev), w)]:
        with pytest.raises(RuntimeError):
            nr(*args)
    with pytest.raises(ValueError):
        rm.edit_distance([[1]], [[1], [2]], device=dev)
    with pytest.raises(ValueError):
        rm.edit_distance([[1] * 1024], [[1]], device=dev)
    with pytest.raises(ValueError):
        rm.word_errors(['a'], ['a'], unit='syllable', device=dev)
    with pytest.raises(ValueError):
        rm.mbr_rerank([[([1], 0.0)] * 129], space=0, device=dev)
    with pytest.raises(ValueError):
        rm.oracle_errors([[1]], [], space=0, device=dev)


# ------------------------------------------------------------------------------------------------ 6. nbest_risk
def _edits(rng, truth, symbols):
    h = list(truth)
    for _ in range(rng.randint(0, 3)):
        kind, at = rng.randint(0, 3), rng.randint(0, len(h) + 1)
        if kind == 0 and h:
            h[min(at, len(h) - 1)] = int(rng.randint(0, symbols))
        elif kind == 1 and h:
            del h[min(at, len(h) - 1)]
        elif kind == 2:
            h.insert(at, int(rng.randint(0, symbols)))
    return h


def _softmax32(scores):
    z = np.asarray(scores, dtype=np.float64)
    z = np.exp(z - z.max())
    return (z / z.sum()).astype(np.float32)


def _risk(dev, groups_of_hyps, weights, gap=0):
    """nbest_risk over lists of token lists -> per group (dmat (K, K), risk (K), pick)"""
    seqs = [h for g in groups_of_hyps for h in g]
    flat, rows = _layout(seqs, gap=gap, fill=None, seed=1)
    groups, at = [], 0
    for g in groups_of_hyps:
        groups.append((at, len(g)))
        at += len(g)
    w = np.concatenate([np.asarray(x, dtype=np.float32) for x in weights])
    dmat, risk, pick = torch.ops.silent_speech.nbest_risk(torch.from_numpy(flat).to(dev), torch.from_numpy(rows).to(dev),
                                                          torch.tensor(groups, dtype=torch.int64).to(dev), torch.from_numpy(w).to(dev))
    dmat, risk, pick = dmat.cpu().numpy(), risk.cpu().numpy(), pick.cpu().numpy()
    assert dmat.shape == (sum(len(g) ** 2 for g in groups_of_hyps),) and risk.dtype == np.float64 and risk.shape == (len(seqs),)
    out, off = [], 0
    for (first, K), p in zip(groups, pick):
        out.append((dmat[off:off + K * K].reshape(K, K), risk[first:first + K], int(p)))
        off += K * K
    return out


def _sizes_case():
    rng = np.random.RandomState(5)
    groups, weights = [], []
    for K in (1, 2, 63, 64, 65, 128, 3):
        truth = rng.randint(0, 3, rng.randint(0, 4)).tolist()
        groups.append([_edits(rng, truth, 3)[:4] for _ in range(K)])
        weights.append(_softmax32(np.sort(rng.randn(K))[::-1] * 2))
    return groups, weights, [oracle.nbest(g, w) for g, w in zip(groups, weights)]


def test_nbest_risk_group_sizes(dev):
    groups, weights, want = _once('sizes', _sizes_case)
    got = _risk(dev, groups, weights, gap=1)
    for (d, r, p), (od, orr, op) in zip(got, want):
        assert np.array_equal(d, d.T) and (np.diag(d) == 0).all() and np.array_equal(d, od)
        assert np.array_equal(r.view(np.int64), orr.view(np.int64))          # bit-equal
        assert p == op


def _mbr_case():
    cases = []
    for seed in range(200):
        rng = np.random.RandomState(seed)
        truth = rng.randint(0, 5, 6).tolist()
        hyps = []
        for _ in range(8):
            h = list(truth)
            for _ in range(rng.randint(0, 3)):
                kind, at = rng.randint(0, 3), rng.randint(0, len(h))
                if kind == 0:
                    h[at] = int(rng.randint(0, 5))
                elif kind == 1 and len(h) > 1:
                    del h[at]
                else:
                    h.insert(at, int(rng.randint(0, 5)))
            hyps.append(h)
        cases.append((hyps, _softmax32(np.sort(rng.randn(8))[::-1])))
    return cases, [oracle.nbest(h, w) for h, w in cases]


def test_nbest_risk_does_not_pass_on_rank_zero(dev):
    cases, want = _once('mbr', _mbr_case)
    moved = sum(1 for _, _, p in want if p != 0)
    assert moved >= len(cases) // 4, moved                               # the oracle's choice leaves rank 0 in at least a quarter of the cases
    got = _risk(dev, [h for h, _ in cases], [w for _, w in cases])
    for (d, r, p), (od, orr, op) in zip(got, want):
        assert np.array_equal(d, od) and np.array_equal(r.view(np.int64), orr.view(np.int64)) and p == op


def test_nbest_risk_ties_and_bad_groups(dev):
    x, y = [1, 2, 3], [1, 4]
    groups = [[x, x, x, x], [x, y, x], [y, x, x], [x], [[], []]]
    weights = [[0.25] * 4, [0.4, 0.2, 0.4], [0.2, 0.4, 0.4], [1.0], [0.5, 0.5]]
    got = _risk(dev, groups, weights)
    assert [p for _, _, p in got] == [0, 0, 1, 0, 0]
    assert (got[0][1] == 0).all() and got[1][1][0] == got[1][1][2] < got[1][1][1] and got[2][1][1] == got[2][1][2] < got[2][1][0]
    for (d, r, p), g, w in zip(got, groups, weights):
        od, orr, op = oracle.nbest(g, w)
        assert np.array_equal(d, od) and np.array_equal(r.view(np.int64), orr.view(np.int64)) and p == op
    # bad entries: a group that leaves the sequence table, a group with a bad sequence in it; the good groups beside them are unaffected
    seqs = [x, y, x, y, y, x, x, y]
    flat, rows = _layout(seqs)
    rows = rows.copy()
    rows[4] = (0, 1024)
    table = [(0, 3), (7, 2), (3, 3), (-1, 2), (6, 2)]
    w = np.asarray([0.5, 0.3, 0.2, 0.6, 0.3, 0.1, 0.25, 0.75], dtype=np.float32)
    dmat, risk, pick = torch.ops.silent_speech.nbest_risk(torch.from_numpy(flat).to(dev), torch.from_numpy(rows).to(dev),
                                                          torch.tensor(table, dtype=torch.int64).to(dev), torch.from_numpy(w).to(dev))
    dmat, risk, pick = dmat.cpu().numpy(), risk.cpu().numpy(), pick.cpu().numpy()
    first, last = oracle.nbest([x, y, x], w[:3]), oracle.nbest([x, y], w[6:])
    assert pick.tolist() == [first[2], -1, -1, -1, last[2]]
    assert np.array_equal(dmat[:9].reshape(3, 3), first[0]) and np.array_equal(dmat[26:30].reshape(2, 2), last[0])
    assert np.array_equal(risk[:3].view(np.int64), first[1].view(np.int64)) and np.array_equal(risk[6:].view(np.int64), last[1].view(np.int64))
    assert np.isnan(risk[3:6]).all()                                       # the group with the bad sequence: NaN risks, its row and column -1
    bad = dmat[13:22].reshape(3, 3)
    assert (bad[1] == -1).all() and (bad[:, 1] == -1).all() and bad[0, 0] == 0 and bad[0, 2] == bad[2, 0] == oracle.distance(y, x)


# ------------------------------------------------------------------------------------------------ 7. the Python surface
WORDS = ['the', 'a', 'cat', 'sat', 'on', 'mat', 'dog', 'ran']


def _sentences(seed, n):
    rng = random.Random(seed)
    return [' '.join(rng.choice(WORDS) for _ in range(rng.randint(0, 9))) for _ in range(n)]


def test_word_errors_cer_and_edit_distance(dev):
    refs, hyps = _sentences(1, 12), _sentences(2, 12)
    we = rm.word_errors(refs, hyps, device=dev)
    assert we.rate == rm.wer(refs, hyps) and we.reference_tokens == sum(len(r.split()) for r in refs)
    ids = {w: k for k, w in enumerate(WORDS)}
    tot = np.zeros(4, dtype=np.int64)
    for r, h, res in zip(refs, hyps, we.per_utterance):
        d, c, _ = oracle.align([ids[w] for w in r.split()], [ids[w] for w in h.split()])
        assert (res.distance, res.hits, res.substitutions, res.deletions, res.insertions) == (d,) + c and res.ops is None
        tot += c
    assert (we.hits, we.substitutions, we.deletions, we.insertions) == tuple(tot)
    chars = sum(oracle.distance([ord(c) for c in r], [ord(c) for c in h]) for r, h in zip(refs, hyps))
    assert rm.cer(refs, hyps, device=dev) == chars / max(sum(len(r) for r in refs), 1)
    res = rm.edit_distance([('x', 1), ['a', 'b', 'c']], [(1, 'x'), ['a', 'c']], ops=True, device=dev)
    assert res[0].distance == 2 and res[0].ops.tolist() == [1, 1] and res[1].ops.tolist() == [0, 2, 0] and res[1].deletions == 1
    assert rm.edit_distance([], [], device=dev) == []
    assert rm.word_errors([], [], device=dev).rate == 0.0


def _split(ints, space):
    words, run = [], []
    for c in list(ints) + [space]:
        if c == space:
            if run:
                words.append(tuple(run))
            run = []
        else:
            run.append(c)
    return words


def test_mbr_rerank_and_oracle_errors_on_beam_search_lists(dev):
    torch.manual_seed(4)
    V, K, space = 5, 8, 0
    T = [9, 1, 7, 12]
    pred = torch.randn(len(T), max(T), V).mul(2.0)
    packed = torch.cat([pred[b, :n] for b, n in enumerate(T)])
    packed = torch.cat([packed, torch.zeros(len(T) * max(T) - packed.shape[0], V)]).reshape(len(T), max(T), V).to(dev)
    lists = rm.beam_decode(packed, T, beam_width=16, n_best=K)
    assert [len(h) for h in lists] == [K, V, K, K]                        # one frame: the empty string and the four labels -- fewer than K
    got = rm.mbr_rerank(lists + [[]], space=space, scale=0.7, device=dev)
    assert got[-1][0] == -1 and got[-1][1].size == 0
    vocab = {}
    for hyps, (pick, risks) in zip(lists, got):
        words = [[vocab.setdefault(w, len(vocab)) for w in _split(ints, space)] for ints, _ in hyps]
        _, orr, op = oracle.nbest(words, _softmax32([0.7 * s for _, s in hyps]))
        assert pick == op and np.array_equal(risks.view(np.int64), orr.view(np.int64))
    chars = rm.mbr_rerank(lists, space=space, unit='char', device=dev)
    for hyps, (pick, risks) in zip(lists, chars):
        _, orr, op = oracle.nbest([ints for ints, _ in hyps], _softmax32([s for _, s in hyps]))
        assert pick == op and np.array_equal(risks.view(np.int64), orr.view(np.int64))
    rng = np.random.RandomState(0)
    refs = [rng.randint(0, V - 1, 8).tolist() for _ in T]
    choices, counts = rm.oracle_errors(refs + [[1, 0, 2]], lists + [[]], space=space, device=dev)
    assert choices[-1] == -1 and counts.per_utterance[-1].deletions == 2
    first = 0
    for ref, hyps, choice, res in zip(refs, lists, choices, counts.per_utterance):
        ds = [oracle.distance([vocab.setdefault(w, len(vocab)) for w in _split(ref, space)], [vocab.setdefault(w, len(vocab)) for w in _split(ints, space)])
              for ints, _ in hyps]
        assert res.distance == min(ds) <= ds[0] and choice == ds.index(min(ds))
        first += ds[0]
    assert counts.substitutions + counts.deletions + counts.insertions <= first + 2
    assert counts.reference_tokens == sum(len(_split(r, space)) for r in refs) + 2


def test_recognition_test_with_mbr_and_details(dev, monkeypatch):
    from silent_speech_amd.architecture import Model
    from tests.test_ctc_beam import _dataset, _references
    ds, m = _dataset(dev, 1 if is_emu(dev) else None)
    seen, real = [], Model.forward_utterances

    def keep(self, raws):
        out = real(self, raws)
        seen.append(out)
        return out
    monkeypatch.setattr(Model, 'forward_utterances', keep)
    kw = dict(batch_size=4, whole_utterances=True, decoder='beam', beam_width=8)
    tt, refs = ds.text_transform, _references(ds)
    det = rm.test(m, ds, dev, details=True, **kw)
    beam = [tt.int_to_text(ints) for logits in seen for ints in rm.beam_decode_utterances(logits, beam_width=8)]
    assert isinstance(det, rm.ErrorCounts) and det.rate == rm.wer(refs, beam) and len(det.per_utterance) == len(ds)
    assert det.reference_tokens == sum(len(r.split()) for r in refs)
    texts = []
    for logits in seen:
        lists = rm.beam_decode_utterances(logits, beam_width=8, n_best=4)
        picks = rm.mbr_rerank(lists, space=tt.chars.index(' '), scale=0.5, device=dev)
        texts += [tt.int_to_text(h[p][0]) for h, (p, _) in zip(lists, picks)]
    got = rm.test(m, ds, dev, mbr=4, mbr_scale=0.5, **kw)
    assert isinstance(got, float) and got == rm.wer(refs, texts)
    with pytest.raises(ValueError):
        rm.test(m, ds, dev, mbr=4)                                         # the greedy decoder has no n-best list
    with pytest.raises(ValueError):
        rm.test(m, ds, dev, mbr=129, **kw)


def test_score_transcripts(dev):
    targets = ['Hello, World!', 'The cat -- sat; on the "mat".', '¿Qué?']
    predictions = ['hello world', 'the cat sat on a mat', 'que']
    got = asr_evaluation.score_transcripts(targets, predictions, device=dev)
    assert asr_evaluation.normalize_transcript(targets[1]) == 'the cat  sat on the mat'
    assert (got.hits, got.substitutions, got.deletions, got.insertions, got.reference_tokens) == (7, 2, 0, 0, 9)
    assert got.rate == 2 / 9 == rm.wer([asr_evaluation.normalize_transcript(t) for t in targets], predictions)

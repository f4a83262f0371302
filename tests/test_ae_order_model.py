"""The definition of the local order of the agglomerate matrices (saamge_amd/ae_order_model.py): the bounds the banded
factorisation needs on the four agglomerates of DESIGN's table under three global numberings, the order-free level
numbering against a sequential Cuthill-McKee with a queue, invariance under translation, and one small case per branch."""
from collections import deque

import numpy as np
import pytest

import ae_order_cases as ac
from saamge_amd import ae_order_model as om

LDS_BAND = 112      # 128 - SB: the widest band the one-launch factorisation holds in LDS (csrc/eig2.hip)

_cases = {}


def case(name):
    if not _cases:
        _cases.update(ac.all_cases())
    return _cases[name]


def is_perm(pos):
    return np.array_equal(np.sort(pos), np.arange(len(pos)))


def bandwidth_by_pairs(pos, adj):
    return max([abs(int(pos[u]) - int(pos[v])) for u in range(len(adj)) for v in adj[u]] or [0])


# ---- a sequential Cuthill-McKee: a queue, neighbours appended by (degree, tie); two sweeps as the model's docstring says ----
def _seq_bfs(root, adj):
    dist = {root: 0}
    q = deque([root])
    while q:
        u = q.popleft()
        for v in adj[u]:
            if int(v) not in dist:
                dist[int(v)] = dist[u] + 1
                q.append(int(v))
    d = max(dist.values())
    return d, min((x for x in dist if dist[x] == d), key=lambda x: (len(adj[x]), rank_of[x]))


rank_of = {}


def sequential_cm(n, adj, rank):
    rank_of.clear()
    rank_of.update({u: int(rank[u]) for u in range(n)})
    pos, posb = [-1] * n, [-1] * n
    nxt = 0
    for start in sorted(range(n), key=lambda u: rank_of[u]):
        if pos[start] >= 0:
            continue
        root = start
        d, cand = _seq_bfs(root, adj)
        for _ in range(om.ROOT_MOVES):
            dc, c2 = _seq_bfs(cand, adj)
            if dc <= d:
                break
            root, d, cand = cand, dc, c2
        end = _seq_sweep(root, adj, rank_of, pos, nxt)
        last = pos.index(end - 1)
        _seq_sweep(last, adj, {u: n - 1 - pos[u] for u in range(n)}, posb, nxt)
        nxt = end
    return np.array(pos), np.array(posb)


def _seq_sweep(root, adj, tie, pos, nxt):
    pos[root] = nxt
    nxt += 1
    q = deque([root])
    while q:
        u = q.popleft()
        for v in sorted((int(v) for v in adj[u] if pos[int(v)] < 0), key=lambda x: (len(adj[x]), tie[x])):
            pos[v] = nxt
            nxt += 1
            q.append(v)
    return nxt


def level_order(n, adj, rank, le):
    """the model's level order: sweep B where it is narrower than sweep A"""
    a, b = om.level_orders(n, adj, rank)
    return b if om.bandwidth(b, le) < om.bandwidth(a, le) else a


TABLE_CASES = ["%s/%s" % (n, k) for n in ac.TABLE for k in ac.NUMBERINGS]


@pytest.mark.parametrize("name", TABLE_CASES)
def test_table_agglomerates_fit_the_lds_band(name):
    dofs, elems = case(name)
    pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
    print(name, "rows", len(dofs), "bw0", bw0, "used", bw, "choice", choice)
    assert is_perm(pos)
    assert bw <= LDS_BAND
    assert bw <= bw0
    assert (choice == 1) == (bw < bw0)
    if bw0 <= om.KEEP_BW:
        assert choice == 0


@pytest.mark.parametrize("seed", range(6))
def test_bound_does_not_hang_on_one_random_numbering(seed):
    # (sweep A alone: 126 on the ball for seed 5, see the model's docstring)
    for name in ("ball_r5", "plate_L_4", "box_9x9x5"):
        pos, bw0, bw, choice = om.ae_order(*ac.table_case(name, ("random", seed)), 1)
        assert choice == 1 and bw <= LDS_BAND and bw0 >= 300, (name, bw0, bw)


@pytest.mark.parametrize("name", sorted(ac.SMALL) + TABLE_CASES)
def test_model_is_sequential_cuthill_mckee_and_reports_its_bandwidths(name):
    dofs, elems = case(name)
    n = len(dofs)
    le = om.local_elems(dofs, elems)
    adj = om.adjacency(n, le)
    rank = om.ranks(dofs)
    a, b = om.level_orders(n, adj, rank)
    sa, sb = sequential_cm(n, adj, rank)
    assert np.array_equal(a, sa) and np.array_equal(b, sb)
    lvl = level_order(n, adj, rank, le)
    pos0 = om.order0(dofs)
    assert is_perm(pos0) and is_perm(a) and is_perm(b)
    assert om.bandwidth(pos0, le) == bandwidth_by_pairs(pos0, adj)
    assert om.bandwidth(lvl, le) == bandwidth_by_pairs(lvl, adj)
    pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
    assert bw0 == bandwidth_by_pairs(pos0, adj) and bw == bandwidth_by_pairs(pos, adj) and bw <= bw0
    assert np.array_equal(pos, lvl if choice else pos0)
    p0, b0, b, c = om.ae_order(dofs, elems, 0)
    assert np.array_equal(p0, pos0) and b0 == bw0 and b == bw0 and c == 0


@pytest.mark.parametrize("name", ["box_9x9x5", "ball_r5", "plate_L_4"])
@pytest.mark.parametrize("kind", ["lexicographic", "refinement"])
def test_translated_copy_gets_the_same_positions(name, kind):
    # (a translation by the coarsest spacing keeps the refinement classes; table order is the same by construction)
    a = ac.table_case(name, kind)
    shift = {"box_9x9x5": (8, 0, 8), "ball_r5": (8, 0, 8), "plate_L_4": (0, 8, 16)}[name]
    if kind == "lexicographic":
        shift = {"box_9x9x5": (3, 2, 7), "ball_r5": (5, 4, 3), "plate_L_4": (1, 3, 9)}[name]
    b = ac.table_case(name, kind, shift=shift)
    ra, rb = om.ae_order(*a, 1), om.ae_order(*b, 1)
    assert np.array_equal(om.ranks(a[0]), om.ranks(b[0]))
    assert np.array_equal(ra[0], rb[0]) and ra[1:] == rb[1:]


def test_the_rule_sees_ranks_only():
    # any increasing map of the global numbers: same level order (the box rule of order 0 is the one place that reads numbers)
    dofs, elems = case("plate_L_4/random")
    m = np.cumsum(np.random.RandomState(1).randint(1, 9, size=int(dofs.max()) + 1))
    d2, e2 = m[dofs], [[int(m[g]) for g in e] for e in elems]
    ra, rb = om.ae_order(dofs, elems, 1), om.ae_order(d2, e2, 1)
    assert ra[3] == 1 and np.array_equal(ra[0], rb[0]) and ra[1:] == rb[1:]


def test_single_dof():
    pos, bw0, bw, choice = om.ae_order(*case("single_dof"), 1)
    assert list(pos) == [0] and (bw0, bw, choice) == (0, 0, 0)


def test_components_are_taken_by_lowest_rank_and_stay_contiguous():
    dofs, elems = case("two_components_and_isolated")
    n = len(dofs)
    adj = om.adjacency(n, om.local_elems(dofs, elems))
    rank = om.ranks(dofs)
    lvl = level_order(n, adj, rank, om.local_elems(dofs, elems))
    comp = {}
    for u in np.argsort(rank):
        if int(u) not in comp:
            stack, comp[int(u)] = [int(u)], len(set(comp.values()))
            while stack:
                x = stack.pop()
                for v in adj[x]:
                    if int(v) not in comp:
                        comp[int(v)] = comp[int(u)]
                        stack.append(int(v))
    ids = np.array([comp[u] for u in range(n)])
    assert ids.max() == 2 and sorted(np.bincount(ids)) == [1, 32, 81]
    assert list(ids[np.argsort(lvl)]) == sorted(ids)      # component 0 (lowest rank) first, each one a contiguous range
    pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
    assert bw0 > om.KEEP_BW and choice == 1               # (so that the device numbers three components)


def test_path_has_depth_n_minus_1_and_band_1():
    dofs, elems = case("path")
    pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
    assert bw0 > om.KEEP_BW and (bw, choice) == (1, 1)


def test_star_keeps_its_order_when_the_level_order_is_no_narrower():
    dofs, elems = case("star")
    n = len(dofs)
    pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
    lvl = level_order(n, om.adjacency(n, om.local_elems(dofs, elems)), om.ranks(dofs), om.local_elems(dofs, elems))
    bw1 = om.bandwidth(lvl, om.local_elems(dofs, elems))
    assert bw0 > om.KEEP_BW and bw1 >= n // 2
    assert choice == (1 if bw1 < bw0 else 0) and bw == min(bw0, bw1)


def test_wide_level_case_has_a_level_of_more_than_256_nodes_and_takes_the_level_order():
    dofs, elems = case("wide_level")
    pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
    assert choice == 1 and bw < bw0
    order = np.argsort(pos)
    adj = om.adjacency(len(dofs), om.local_elems(dofs, elems))
    level, d = om._bfs(int(order[0]), adj, len(dofs))
    assert np.bincount(level).max() > 256


def test_more_than_256_rows_and_mixed_and_coarse_shapes_take_the_level_order():
    for name in ("rows_over_256", "mixed_sizes", "coarse_chain"):
        dofs, elems = case(name)
        pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
        assert bw0 > om.KEEP_BW and choice == 1 and bw < bw0, name
    assert len(case("rows_over_256")[0]) > 256
    assert len({len(e) for e in case("mixed_sizes")[1]}) >= 3


def test_coarse_pair_is_two_cliques():
    dofs, elems = case("coarse_pair")
    pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
    assert len(dofs) == 50 and bw0 <= 49
    assert choice == 0          # 50 rows: bw0 <= 49 <= 51, left alone


def test_box_under_the_narrowest_window_is_left_alone():
    dofs, elems = case("box_left_alone")
    pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
    assert bw0 <= om.KEEP_BW and choice == 0 and bw == bw0
    assert np.array_equal(pos, om.order0(dofs))


def test_headline_box_keeps_the_box_rule():
    dofs, elems = case("box_9x9x5/lexicographic")
    pos, bw0, bw, choice = om.ae_order(dofs, elems, 1)
    assert (bw0, bw, choice) == (51, 51, 0)


def test_bad_mode_is_refused():
    with pytest.raises(ValueError):
        om.ae_order(*case("single_dof"), 2)

"""CPU model of the local order of the agglomerate matrices (csrc/assemble.hip: ae_perm_kernel, ae_level_order_kernel) --
numpy only, test infrastructure like capi.py.

This file is the DEFINITION of the result: the device code restates it and must give the same integers.

Input for one agglomerate: `dofs`, its global dof numbers in table order (local row r is dofs[r]), and `elems`, the dof lists
of the elements of the agglomerate (global numbers; every entry is one of `dofs`).

  graph      two rows are adjacent when an element of the agglomerate holds both; a row is not its own neighbour.
  rank       rank of the row's global number among `dofs`.
  degree     number of distinct neighbours.
  order 0    today's order (ae_perm_kernel): position = rank -- unless the sorted dofs form a lexicographic box
             g0 + i + s2 j + s3 k (0 <= i < a, 0 <= j < b, 0 <= k < c, s2 >= a, s3 >= b s2 where c > 1), whose shortest
             extent then runs fastest.  This is the only place that looks at global numbers, and a translation keeps it.
  bandwidth  structural half bandwidth of an order: the largest |pos[u] - pos[v]| over adjacent u, v (0 without edges).
  level      ranks and degrees only.  Components are taken by lowest unnumbered rank.  Root of a component: start at its
  order      lowest rank r and run a breadth-first search, depth d.  The candidate c is the node of the LAST level with
             the smallest (degree, rank).  At most ROOT_MOVES (8) times: search from c; if its depth is greater than d,
             c becomes the root, d its depth and c its search's candidate; otherwise stop.  Numbering (a sweep): the root
             takes the component's first free position; then level by level, the nodes of a level sorted by (position of
             their lowest-positioned neighbour in the previous level, degree, tie) take the next positions.  Keys never
             tie (the tie key is a permutation).  This is Cuthill-McKee with neighbours appended by (degree, tie) --
             tests/test_ae_order_model.py holds it to the sequential textbook form.  No reversal: it does not change a
             bandwidth.
             Two sweeps per component.  Sweep A starts at the root with tie = rank.  Sweep B starts at the node sweep A
             numbered LAST, over the same positions, with tie = n - 1 - (position in sweep A): where degree and parent
             do not decide, the nodes follow sweep A backwards.  (Sweep A alone does not hold the bound.  With ranks from
             a random numbering its ties fall at random: over 16 random numberings the ball of radius 5 got 101 .. 126
             and the L-shaped plate 56 .. 92, against the 112 the LDS factorisation holds.  Sweep B gave 101 on the ball
             under every numbering tried, 89 on the 9 x 9 x 5 box, at most 79 on the plate: its ties come from an order
             that is already a coherent sweep through the agglomerate.)  The level order of the agglomerate is A's
             positions or B's, all components together: B if its bandwidth is smaller than A's, otherwise A.
  choice     bw0 = bandwidth of order 0.  If bw0 <= KEEP_BW (51 = 67 - SB, the narrowest LDS window of the banded
             factorisation) order 0 stays and nothing else is computed.  An agglomerate of more than MAX_ROWS (4096) rows
             keeps order 0 as well: the device packs (degree, rank) into 12 bits each.  Otherwise the level order is
             computed with its bandwidth bw1 and is used if bw1 < bw0.

ae_order(dofs, elems, mode) returns (pos, bw0, bw, choice): pos[r] the position of local row r, bw the bandwidth of the
order that was taken, choice 1 for the level order.  mode 0: order 0 always (bw = bw0, choice = 0).
"""
import numpy as np

KEEP_BW = 51
MAX_ROWS = 4096
ROOT_MOVES = 8


def local_elems(dofs, elems):
    """the elements' dof lists in local row numbers"""
    dofs = np.asarray(dofs, np.int64)
    loc = {int(g): r for r, g in enumerate(dofs)}
    assert len(loc) == len(dofs), "an agglomerate lists a dof twice"
    return [np.array([loc[int(g)] for g in e], np.int64) for e in elems]


def adjacency(n, lelems):
    """sorted neighbour arrays of every local row"""
    nb = [set() for _ in range(n)]
    for e in lelems:
        for u in e:
            nb[int(u)].update(int(v) for v in e)
    return [np.array(sorted(nb[u] - {u}), np.int64) for u in range(n)]


def ranks(dofs):
    dofs = np.asarray(dofs, np.int64)
    rank = np.empty(len(dofs), np.int64)
    rank[np.argsort(dofs, kind="stable")] = np.arange(len(dofs))
    return rank


def order0(dofs, box_order=True):
    """ae_perm_kernel: pos[r] of local row r"""
    dofs = np.asarray(dofs, np.int64)
    n = len(dofs)
    rank = ranks(dofs)
    sid = np.sort(dofs)
    a = 1
    while a < n and sid[a] == sid[0] + a:
        a += 1
    b, c, s2, s3, ok = 1, 1, 0, 0, False
    if box_order and a < n and n % a == 0:
        s2 = sid[a] - sid[0]
        while b * a < n and sid[b * a] == sid[0] + b * s2:
            b += 1
        if n % (a * b) == 0:
            c = n // (a * b)
            s3 = sid[a * b] - sid[0] if c > 1 else 0
            ok = s2 >= a and (c == 1 or s3 >= b * s2)
    if ok:
        idx = np.arange(n)
        i, j, k = idx % a, (idx // a) % b, idx // (a * b)
        ok = bool((sid == sid[0] + i + s2 * j + s3 * k).all())
    if not ok:
        return rank
    ext, dim = [a, b, c], [0, 1, 2]
    for u in range(2):                      # the kernel's bubble sort: ties keep their order
        for v in range(2 - u):
            if ext[v] > ext[v + 1]:
                ext[v], ext[v + 1] = ext[v + 1], ext[v]
                dim[v], dim[v + 1] = dim[v + 1], dim[v]
    crd = [rank % a, (rank // a) % b, rank // (a * b)]
    return crd[dim[0]] + ext[0] * (crd[dim[1]] + ext[1] * crd[dim[2]])


def bandwidth(pos, lelems):
    """every pair of an element is adjacent: the spread of the positions of an element, the largest over the elements"""
    bw = 0
    for e in lelems:
        if len(e):
            p = pos[e]
            bw = max(bw, int(p.max() - p.min()))
    return bw


def _bfs(root, adj, n):
    level = np.full(n, -1, np.int64)
    level[root] = 0
    front, d = [root], 0
    while True:
        nxt = sorted({int(v) for u in front for v in adj[u] if level[v] < 0})
        if not nxt:
            return level, d
        d += 1
        level[nxt] = d
        front = nxt


def _candidate(level, d, deg, rank):
    last = np.flatnonzero(level == d)
    return int(last[np.lexsort((rank[last], deg[last]))[0]])


def _sweep(root, level, d, adj, deg, tie, pos, nxt):
    """numbers the component of `root` (its breadth-first levels given) from position nxt on; returns the next free one"""
    pos[root] = nxt
    nxt += 1
    for lv in range(1, d + 1):
        nodes = np.flatnonzero(level == lv)
        first = np.array([min(pos[v] for v in adj[u] if level[v] == lv - 1) for u in nodes], np.int64)
        for u in nodes[np.lexsort((tie[nodes], deg[nodes], first))]:
            pos[u] = nxt
            nxt += 1
    return nxt


def level_orders(n, adj, rank):
    """(positions of sweep A, positions of sweep B)"""
    deg = np.array([len(a) for a in adj], np.int64)
    pos = np.full(n, -1, np.int64)
    posb = np.full(n, -1, np.int64)
    byrank = np.argsort(rank)
    nxt = 0
    for start in byrank:                    # components by lowest unnumbered rank
        if pos[start] >= 0:
            continue
        root = int(start)
        level, d = _bfs(root, adj, n)
        cand = _candidate(level, d, deg, rank)
        for _ in range(ROOT_MOVES):
            lc, dc = _bfs(cand, adj, n)
            if dc <= d:
                break
            root, d, level = cand, dc, lc
            cand = _candidate(level, d, deg, rank)
        end = _sweep(root, level, d, adj, deg, rank, pos, nxt)
        last = int(np.flatnonzero(pos == end - 1)[0])
        lb, db = _bfs(last, adj, n)
        _sweep(last, lb, db, adj, deg, n - 1 - pos, posb, nxt)
        nxt = end
    assert nxt == n
    return pos, posb


def ae_order(dofs, elems, mode=1):
    """(pos, bw0, bw, choice) of one agglomerate, see the module's docstring"""
    if mode not in (0, 1):
        raise ValueError("ae_order must be 0 or 1")
    dofs = np.asarray(dofs, np.int64)
    n = len(dofs)
    le = local_elems(dofs, elems)
    pos0 = np.asarray(order0(dofs), np.int64)
    bw0 = bandwidth(pos0, le)
    if mode == 0 or bw0 <= KEEP_BW or n > MAX_ROWS:
        return pos0, bw0, bw0, 0
    posa, posb = level_orders(n, adjacency(n, le), ranks(dofs))
    bwa, bwb = bandwidth(posa, le), bandwidth(posb, le)
    pos1, bw1 = (posb, bwb) if bwb < bwa else (posa, bwa)
    if bw1 < bw0:
        return pos1, bw0, bw1, 1
    return pos0, bw0, bw0, 0

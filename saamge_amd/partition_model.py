"""CPU model of the device partitioner (csrc/partition.hip) -- numpy only, test infrastructure like capi.py.

This file is the DEFINITION of the algorithm: the device code restates it and must give the same integers.  Every step is
a minimum / maximum / count over integers, so no result depends on an execution order.

  priority     prio(i) = fmix32(i + seed * 0x9E3779B9): a bijection of 32-bit integers, so priorities never tie.
  element graph  e != f adjacent when they share >= min_shared dofs; symmetric CSR, no self-loops, columns ascending.
               An element that lists a dof twice is refused.
  seeding      `reseed`: inside every flagged part p the k[p] nodes of lowest priority become seeds; the lowest keeps the
               label p, the r-th lowest (r >= 1) gets nlabels + off[p] + r - 1 with off the exclusive sum of k - 1 over the
               flagged parts in label order.  The first seeding is this with one part 0 holding every node and
               k = target = ceil(n / elems_per_agg).  This is `seeding = 0`.
  spaced seeds `seeding = 1` replaces the FIRST seeding only (the reseeding of oversized parts stays as above).  dist(u, v) is
               the hop distance (self-loops ignored, other components infinitely far); a set is r-independent when all its
               pairs have dist > r.
               greedy   the greedy r-independent set given a fixed set F: walk the nodes in ascending priority; a node
                        joins when no member so far, F included, lies within r hops.  Priorities never tie, so the set is
                        unique.  S_r is this set with F empty; S_0 is every node.
               radius   target = ceil(n / elems_per_agg); r = the smallest radius >= 1 with |S_r| <= target, and
                        RADIUS_MAX = 32 when there is none (more components than targets, or a component of larger
                        diameter: S_32 is kept, and the stalled-growth rule below seeds a component that got no seed).
               top-up   when |S_r| < target: E = the greedy (r - 1)-independent extension of F = S_r; the
                        target - |S_r| members of E of lowest priority are added, all of E if there are fewer.  For r = 1
                        every node outside S_1 is in E and the top-up is by priority alone.  The seed count is
                        min(target, |S_r| + |E|) (|S_r| when that is above the target); first-stage seeds are pairwise more
                        than r hops apart, all seeds more than r - 1.
               labels   the seeds sorted by priority get 0, 1, 2, ... as in the first seeding above.
               fixed point (the form the device runs, `independent_set_fixed_point`): nodes are undecided, seed or out.
                        One round: every node takes the minimum priority of the UNDECIDED nodes within r hops (r pull sweeps
                        over closed neighbourhoods, passing through nodes of every state); an undecided node that holds its
                        own priority becomes a seed; every undecided node within r hops of a new seed becomes out (r sweeps
                        of a flag).  Until nobody is undecided.  With F: its members are no candidates and the nodes within
                        r hops of it start as out.  This is the greedy set: an undecided node that is the minimum of its
                        ball has every lower-priority node of that ball already out.
  growth       level-synchronous pull: every unlabelled node with a labelled neighbour (of the same `dom`, when given) takes
               the smallest such label of the PREVIOUS round.  Nothing changed and nodes are left: the unlabelled node of
               lowest priority becomes a seed with the next free label.  This is `growth = 0`.
  balanced growth  `growth = 1` replaces the growth after the first seeding (either `seeding`) and the regrowth after each
               recentring pass; the regrowth inside the size repair (`dom`) stays level-synchronous.  cap = elems_per_agg.
               round    size[p] from the labels of the previous round; p is OPEN while size[p] < cap, its quota is
                        cap - size[p].  Every unlabelled node u with a neighbour in an open part is a claimant of c(u), the
                        smallest such label; hits(u) = the number of u's neighbours labelled c(u), clipped to HITS_MAX =
                        65 535.  The claimants of p in the order (hits descending, priority ascending): the first quota[p]
                        are labelled p, the others stay unlabelled.  Priorities never tie, so the choice is unique.
               release  a round without claimant while nodes are unlabelled: the rest is labelled by the growth above,
                        from all labels as they stand, its rule for a stalled component included.
               counts   (`growth_info`) balanced rounds = the rounds that had a claimant (each labels a node); nodes
                        labelled under a quota; parts open at the release and nodes unlabelled at it (0 and 0 when there
                        was no release).  With recentring they are those of the last growth.
               A node joins a part only through a neighbour already in it, so parts stay connected.  No part exceeds cap
               before the release (a round adds at most cap - size[p] to p).  Every step is a minimum, a count or a rank
               in a strict order, so nothing depends on an execution order.
  recentring   depth = hops to the nearest node of the own part that has a neighbour in another part, over same-label edges.
               New seed of a part = its node of largest depth, ties to the lowest priority; a part without boundary keeps
               its seed.  Labels stay with their parts; growth restarts from the new seeds.
  size repair  (a) while a part is larger than max_size, at most REPAIR_ROUNDS times: reseed it with
               max(2, ceil(size / elems_per_agg)) seeds and grow across same-old-label edges only.  Every flagged part is
               connected and gets two seeds or more, so its pieces are strictly smaller; on meshes a few rounds reach the
               cap.  A hub with very many leaves shrinks by about one piece per round: the bound ends that, and a part
               still above the cap after it is left as it is.
               (b) rounds: a part p smaller than min_size PROPOSES to its adjacent part q of smallest (size, label) among
               those with size[p] + size[q] <= max_size.  Proposals can only cycle in pairs (the choice is a strict
               minimum), so: q is STATIONARY when it proposes nothing, or proposes to a part that proposes back and has the
               larger label.  p joins q when q is stationary, p is not, and p is the proposer of q with the smallest
               (size, label).  One joiner per part and round keeps the cap.  Until a round merges nothing, at most 8.
  refine       `refine_graph`, `refine_rounds > 0`: boundary refinement, off by default.  It takes any partition (labels in
               [0, nparts), no part empty) and works after the merges, before the renumbering, with the resolved caps
               (max_size 0: no cap; floor = max(min_size, 1)).  Entries u == v are ignored throughout; deg(v) is the number
               of entries of row v.  One round, from the labels and sizes of the previous round:
               counts   v in part p: own(v) = its neighbours labelled p, c_q(v) = those labelled q != p.  The target t(v) is
                        the q of largest c_q, ties to the smallest label; gain(v) = c_t - own.
               candidate  gain > 0, own >= 1, size[t] < max_size (with a cap), size[p] > floor, deg(v) <= REFINE_DEG_MAX =
                        1024, and v is FREE.
               free     N = the neighbours of v labelled p.  Not free when own = 0 or own > REFINE_LOCAL_MAX = 64.  Two members
                        of N are linked when they are adjacent or have a common neighbour x != v labelled p; v is free when N
                        is connected under the transitive closure of the links (|N| = 1 is).  The two-hop link matters: a face
                        graph of hexes has no triangles, and only leaves could move without it.
               winners  key(v) = ((65535 - min(gain, 65535)) << 32) | prio(v); a candidate wins when its key is the minimum
                        over the candidates within 2 hops (closed balls through nodes of every kind; one pass, not iterated).
               quotas   the winners per target in the order (clipped gain descending, priority ascending): the first
                        max_size - size[t] are admitted (all without a cap); the admitted per source in the same order: the
                        first size[p] - floor move (`select_claimants` twice).
               apply    the movers take their target's label.
               The pass stops when a round has no candidate or when `rounds` rounds have moved nodes.  info = [rounds that
               moved nodes, nodes moved, sum of the gains = cut edges removed, 1 if it stopped for want of a candidate].
               Why it holds together:
               - winners are pairwise more than 2 hops apart (of two candidates within 2 hops only the smaller key can be the
                 minimum of its ball), so movers are never adjacent and each move lowers the cut by exactly its gain;
               - the cut falls by >= 1 in every round that moves a node, so the pass ends;
               - a round with a candidate moves a node: the candidate of smallest key wins its ball, is first in its target's
                 order (quota >= 1, size[t] < max_size) and first in its source's (quota >= 1, size[p] > floor);
               - a connected part stays connected: the members of N and the nodes x that link them lie within 2 hops of the
                 mover v, so none of them moves in this round; a path of the part through v enters and leaves it by members
                 of N and is rerouted through N and the linking nodes;
               - a joiner stays attached: gain > 0 and own >= 1 give c_t >= 2 neighbours in the target, and they stay;
               - sizes hold: at most max_size - size[t] nodes join t and at most size[p] - floor leave p, so no part is
                 emptied, exceeds max_size or falls below floor through the pass; the part count stays.
  renumbering  parts 0 .. nparts-1 in the order of their smallest member.
  quotient     parts adjacent when any of their members are; unweighted, columns ascending.
"""
import numpy as np

MERGE_ROUNDS = 8
REPAIR_ROUNDS = 32
DEFAULT_LLOYD_ITERS = 0
RADIUS_MAX = 32
HITS_MAX = 65535
REFINE_DEG_MAX = 1024
REFINE_LOCAL_MAX = 64
GAIN_MAX = 65535


def priority(n, seed=0):
    x = (np.arange(n, dtype=np.uint64) + np.uint64((int(seed) * 0x9E3779B9) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.int64)


def resolve_sizes(elems_per_agg, max_size=-1, min_size=-1):
    if max_size < 0:
        max_size = 2 * elems_per_agg
    if min_size < 0:
        min_size = elems_per_agg // 4
    return int(max_size), int(min_size)


def build_element_graph(elem_ptr, elem_to_dof, ND, min_shared=1):
    """elem_ptr (NE + 1), flat elem_to_dof -> (xadj int64 (NE + 1), adj int32)."""
    elem_ptr = np.asarray(elem_ptr, np.int64)
    e2d = np.asarray(elem_to_dof, np.int64)
    NE = len(elem_ptr) - 1
    elem = np.repeat(np.arange(NE, dtype=np.int64), np.diff(elem_ptr))
    if len(np.unique(elem * max(int(ND), 1) + e2d)) != len(e2d):
        raise ValueError("an element lists a dof twice")
    order = np.argsort(e2d, kind="stable")
    dofs, elems = e2d[order], elem[order]
    cnt = np.bincount(dofs, minlength=ND)
    start = np.concatenate([[0], np.cumsum(cnt)])
    keys = []
    for c in np.unique(cnt):
        if c < 2:
            continue
        d = np.flatnonzero(cnt == c)
        lists = elems[start[d][:, None] + np.arange(c)[None, :]]          # (m, c)
        keys.append((lists[:, :, None] * NE + lists[:, None, :]).ravel())
    if keys:
        k, shared = np.unique(np.concatenate(keys), return_counts=True)
        e, f = k // NE, k % NE
        keep = (e != f) & (shared >= min_shared)
        e, f = e[keep], f[keep]
    else:
        e = f = np.zeros(0, np.int64)
    xadj = np.concatenate([[0], np.cumsum(np.bincount(e, minlength=NE))]).astype(np.int64)
    return xadj, f.astype(np.int32)


class _Graph(object):
    def __init__(self, n, xadj, adj):
        self.n = int(n)
        self.xadj = np.asarray(xadj, np.int64)
        self.dst = np.asarray(adj, np.int64)
        self.src = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.xadj))
        self.rows = np.flatnonzero(np.diff(self.xadj) > 0)          # the rows that have entries


def _grow(g, label, isseed, prio, nlabels, dom=None):
    BIG = np.iinfo(np.int64).max
    same = np.ones(len(g.src), bool) if dom is None else dom[g.src] == dom[g.dst]
    while True:
        unl = label < 0
        if not unl.any():
            return label, nlabels
        m = same & unl[g.src] & (label[g.dst] >= 0)
        if m.any():
            new = np.full(g.n, BIG)
            np.minimum.at(new, g.src[m], label[g.dst[m]])
            label = np.where(new < BIG, new, label)
        else:
            u = np.flatnonzero(unl)
            s = u[np.argmin(prio[u])]
            label = label.copy()
            label[s] = nlabels
            isseed[s] = True
            nlabels += 1


def select_claimants(claim, hits, prio, quota):
    """claim[u] = c(u) or -1.  Per part the quota[p] claimants first in (hits clipped descending, priority ascending)."""
    nodes = np.flatnonzero(claim >= 0)
    h = np.minimum(hits[nodes], HITS_MAX)
    order = np.lexsort((prio[nodes], -h, claim[nodes]))
    nodes = nodes[order]
    lab = claim[nodes]
    rank = np.arange(len(nodes)) - np.searchsorted(lab, lab, side="left")
    chosen = np.zeros(len(claim), bool)
    chosen[nodes[rank < quota[lab]]] = True
    return chosen


def _grow_balanced(g, label, isseed, prio, nlabels, cap, info, hook=None):
    """`growth = 1`.  info (a list of 4) receives the counts; hook(label, nlabels) sees the labels before the release."""
    BIG = np.iinfo(np.int64).max
    info[:] = [0, 0, 0, 0]
    while True:
        unl = label < 0
        if not unl.any():
            break
        size = np.bincount(label[~unl], minlength=nlabels)
        lab_dst = label[g.dst]
        m = unl[g.src] & (lab_dst >= 0)
        m[m] = size[lab_dst[m]] < cap
        if not m.any():
            info[2], info[3] = int((size < cap).sum()), int(unl.sum())
            break
        c = np.full(g.n, BIG)
        np.minimum.at(c, g.src[m], lab_dst[m])
        claim = np.where(c < BIG, c, -1)
        e = (claim[g.src] >= 0) & (lab_dst == claim[g.src])
        hits = np.bincount(g.src[e], minlength=g.n)
        chosen = select_claimants(claim, hits, prio, cap - size)
        label = np.where(chosen, claim, label)
        info[0] += 1
        info[1] += int(chosen.sum())
    if hook is not None:
        hook(label.copy(), nlabels)
    return _grow(g, label, isseed, prio, nlabels)


def _reseed(g, label, isseed, prio, nlabels, k):
    """k[p] > 0 flags part p.  Returns the labels with the flagged parts cleared down to their new seeds."""
    flagged = k > 0
    off = np.concatenate([[0], np.cumsum(np.where(flagged, k - 1, 0))])
    order = np.lexsort((prio, label))
    sizes = np.bincount(label, minlength=nlabels)
    start = np.concatenate([[0], np.cumsum(sizes)])
    dom_sorted = label[order]
    rank = np.arange(g.n) - start[dom_sorted]
    out = label.copy()
    infl = flagged[label]
    out[infl] = -1
    isseed[infl] = False
    sel = flagged[dom_sorted] & (rank < k[dom_sorted])
    nodes, p, r = order[sel], dom_sorted[sel], rank[sel]
    out[nodes] = np.where(r == 0, p, nlabels + off[p] + r - 1)
    isseed[nodes] = True
    return out, nlabels + int(off[-1])


def _ball_step(g, x, op):
    """x over closed neighbourhoods: op = np.minimum / np.logical_or, one hop."""
    out = x.copy()
    if len(g.rows):
        out[g.rows] = op(out[g.rows], op.reduceat(x[g.dst], g.xadj[g.rows]))
    return out


def independent_set_greedy(g, prio, r, fixed=None):
    """The definition: nodes in ascending priority, each joins when no member or node of `fixed` lies within r hops.
    Returns the members in ascending node order."""
    blocked = np.zeros(g.n, bool)

    def block(v):
        blocked[v] = True
        seen, front = {v}, [v]
        for _ in range(r):
            nxt = []
            for w in front:
                for u in g.dst[g.xadj[w]:g.xadj[w + 1]].tolist():
                    if u not in seen:
                        seen.add(u)
                        nxt.append(u)
            blocked[nxt] = True
            front = nxt

    if fixed is not None:
        for v in fixed:
            block(int(v))
    members = []
    for v in np.argsort(prio[:g.n], kind="stable"):
        if not blocked[v]:
            members.append(int(v))
            block(int(v))
    return np.sort(np.array(members, np.int64))


def independent_set_fixed_point(g, prio, r, fixed=None):
    """The same set by rounds that do not depend on an order.  Returns (members ascending, rounds)."""
    BIG = np.iinfo(np.int64).max
    UNDECIDED, SEED, OUT = 0, 1, 2
    state = np.zeros(g.n, np.int8)
    if fixed is not None and len(fixed):
        flag = np.zeros(g.n, bool)
        flag[fixed] = True
        for _ in range(r):
            flag = _ball_step(g, flag, np.logical_or)
        state[flag] = OUT
        state[fixed] = OUT
    rounds = 0
    while (state == UNDECIDED).any():
        rounds += 1
        key = np.where(state == UNDECIDED, prio, BIG)
        for _ in range(r):
            key = _ball_step(g, key, np.minimum)
        new = (state == UNDECIDED) & (key == prio)
        flag = new
        for _ in range(r):
            flag = _ball_step(g, flag, np.logical_or)
        state[flag & (state == UNDECIDED)] = OUT
        state[new] = SEED
    return np.flatnonzero(state == SEED), rounds


def spaced_seeds(g, prio, target, greedy=False):
    """`seeding = 1`: dict(radius, first = S_r, ext = E, seeds, rounds); node arrays ascending.  greedy = True runs the
    sequential definition in place of the fixed point (rounds = 0)."""
    def indep(r, fixed=None):
        if greedy:
            return independent_set_greedy(g, prio, r, fixed), 0
        return independent_set_fixed_point(g, prio, r, fixed)

    rounds = 0
    for r in range(1, RADIUS_MAX + 1):
        first, k = indep(r)
        rounds += k
        if len(first) <= target:
            break
    ext = np.zeros(0, np.int64)
    seeds = first
    if len(first) < target:
        ext, k = indep(r - 1, first)
        rounds += k
        add = ext[np.argsort(prio[ext], kind="stable")[:target - len(first)]]
        seeds = np.sort(np.concatenate([first, add]))
    return dict(radius=r, first=first, ext=ext, seeds=seeds, rounds=rounds)


def _recentre(g, label, isseed, prio, nlabels):
    bnd = np.zeros(g.n, bool)
    bnd[g.src[label[g.src] != label[g.dst]]] = True
    depth = np.where(bnd, 0, -1).astype(np.int64)
    same = label[g.src] == label[g.dst]
    d = 0
    while True:
        d += 1
        m = same & (depth[g.src] < 0) & (depth[g.dst] == d - 1)
        if not m.any():
            break
        depth[g.src[m]] = d
    submit = (depth >= 0) | isseed
    key = ((depth + 1) << 32) | (0xFFFFFFFF - prio)
    best = np.full(nlabels, -1, np.int64)
    np.maximum.at(best, label[submit], key[submit])
    newseed = submit & (key == best[label])
    isseed[:] = newseed
    return np.where(newseed, label, -1)


def _merge_round(g, label, nlabels, max_size, min_size):
    BIG = np.iinfo(np.int64).max
    sizes = np.bincount(label, minlength=nlabels)
    lp, lq = label[g.src], label[g.dst]
    m = (lp != lq) & (sizes[lp] < min_size)
    if max_size > 0:
        m &= sizes[lp] + sizes[lq] <= max_size
    prop = np.full(nlabels, BIG)
    np.minimum.at(prop, lp[m], (sizes[lq[m]] << 32) | lq[m])
    has = prop < BIG
    q = np.where(has, prop & 0xFFFFFFFF, -1)
    qs = np.where(has, q, 0)
    stationary = ~has | ((q[qs] == np.arange(nlabels)) & (np.arange(nlabels) < q))
    win = np.full(nlabels, BIG)
    p = np.flatnonzero(has)
    np.minimum.at(win, q[p], (sizes[p] << 32) | p)
    join = has & ~stationary & stationary[qs] & ((win[qs] & 0xFFFFFFFF) == np.arange(nlabels))
    target = np.where(join, q, np.arange(nlabels))
    return target[label], int(join.sum())


def renumber(label, nlabels):
    n = len(label)
    minid = np.full(nlabels, n, np.int64)
    np.minimum.at(minid, label, np.arange(n))
    first = minid[label] == np.arange(n)
    rank = np.cumsum(first) - first
    newnum = np.zeros(nlabels, np.int64)
    newnum[label[first]] = rank[first]
    return newnum[label].astype(np.int32), int(first.sum())


def _expand_rows(xadj, rows):
    """(owner, pos): for every entry of the rows given, the index into `rows` and the position in the CSR arrays."""
    cnt = xadj[rows + 1] - xadj[rows]
    owner = np.repeat(np.arange(len(rows), dtype=np.int64), cnt)
    first = np.cumsum(cnt) - cnt
    pos = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first, cnt) + np.repeat(xadj[rows], cnt)
    return owner, pos


def refine_counts(g, label, nparts):
    """own, target (-1: no foreign neighbour), c_target per node; entries u == v ignored."""
    nl = g.src != g.dst
    src, ls, ld = g.src[nl], label[g.src[nl]], label[g.dst[nl]]
    own = np.bincount(src[ls == ld], minlength=g.n)
    f = ls != ld
    k, cnt = np.unique(src[f] * nparts + ld[f], return_counts=True)
    v, q = k // nparts, k % nparts
    order = np.lexsort((q, -cnt, v))
    v, q, cnt = v[order], q[order], cnt[order]
    first = np.ones(len(v), bool)
    first[1:] = v[1:] != v[:-1]
    target = np.full(g.n, -1, np.int64)
    ct = np.zeros(g.n, np.int64)
    target[v[first]] = q[first]
    ct[v[first]] = cnt[first]
    return own, target, ct


def refine_free(g, label, nodes):
    """free(v) for the nodes given (each with 1 <= own).  The members (v, a) of N(v) and the nodes (v, x), x != v of v's part
    adjacent to a member, form a graph with the edges member -- adjacent node; N(v) is connected under the closure of the
    links exactly when its members lie in one component of it."""
    n = g.n
    nodes = np.asarray(nodes, np.int64)
    if not len(nodes):
        return np.zeros(0, bool)
    ci, pos = _expand_rows(g.xadj, nodes)
    a = g.dst[pos]
    keep = (label[a] == label[nodes[ci]]) & (a != nodes[ci])
    mk = np.unique(ci[keep] * n + a[keep])
    ci, a = mk // n, mk % n
    ei, pos = _expand_rows(g.xadj, a)
    x = g.dst[pos]
    keep = (label[x] == label[a[ei]]) & (x != nodes[ci[ei]])
    ei, x = ei[keep], x[keep]
    allk, inv = np.unique(np.concatenate([mk, ci[ei] * n + x]), return_inverse=True)
    inv = inv.ravel()
    u, w = inv[:len(mk)][ei], inv[len(mk):]
    comp = np.arange(len(allk), dtype=np.int64)
    while True:
        new = comp.copy()
        np.minimum.at(new, u, comp[w])
        np.minimum.at(new, w, comp[u])
        new = new[new]
        if (new == comp).all():
            break
        comp = new
    cm = comp[inv[:len(mk)]]
    lo = np.full(len(nodes), np.iinfo(np.int64).max)
    hi = np.full(len(nodes), -1, np.int64)
    np.minimum.at(lo, ci, cm)
    np.maximum.at(hi, ci, cm)
    return lo == hi


def refine_round(g, label, nparts, prio, max_size, floor):
    """One round: (new labels, stats).  stats counts what every rule of the round did (the tests read them)."""
    BIG = np.iinfo(np.int64).max
    size = np.bincount(label, minlength=nparts)
    own, target, ct = refine_counts(g, label, nparts)
    gain = ct - own
    ts = np.where(target >= 0, target, 0)
    gainer = (target >= 0) & (gain > 0) & (own >= 1)
    ok_size = size[label] > floor
    if max_size > 0:
        ok_size &= size[ts] < max_size
    ok_deg = np.diff(g.xadj) <= REFINE_DEG_MAX
    ok_local = own <= REFINE_LOCAL_MAX
    pre = gainer & ok_size & ok_deg & ok_local
    nodes = np.flatnonzero(pre)
    free = refine_free(g, label, nodes)
    cand = np.zeros(g.n, bool)
    cand[nodes[free]] = True
    st = dict(gainers=int(gainer.sum()), size_refused=int((gainer & ~ok_size).sum()),
              deg_refused=int((gainer & ok_size & ~ok_deg).sum()),
              local_refused=int((gainer & ok_size & ok_deg & ~ok_local).sum()), not_free=int(len(nodes) - free.sum()),
              candidates=int(cand.sum()), winners=0, admitted=0, movers=0, gain=0)
    if not st["candidates"]:
        return label, st
    key = np.where(cand, ((GAIN_MAX - np.minimum(gain, GAIN_MAX)) << 32) | prio, BIG)
    ball = _ball_step(g, _ball_step(g, key, np.minimum), np.minimum)
    win = cand & (ball == key)
    quota = np.full(nparts, BIG) if max_size <= 0 else max_size - size
    adm = select_claimants(np.where(win, target, -1), gain, prio, quota)
    move = select_claimants(np.where(adm, label, -1), gain, prio, size - floor)
    st.update(winners=int(win.sum()), admitted=int(adm.sum()), movers=int(move.sum()), gain=int(gain[move].sum()))
    return np.where(move, target, label), st


def refine_graph(n, xadj, adj, part, nparts, rounds, max_size, min_size, seed=0, info=None, hook=None):
    """The refinement pass on any partition: labels in [0, nparts), no part empty; max_size 0: no cap.  Returns the labels
    (int32, the caller's numbering).  info (a list of 4) receives [rounds that moved nodes, nodes moved, sum of the gains,
    stopped for want of a candidate]; hook(label, stats) is called after every round, the one without candidate included."""
    if rounds < 0 or max_size < 0 or min_size < 0:
        raise ValueError("rounds, max_size and min_size >= 0")
    label = np.asarray(part, np.int64).copy()
    if len(label) != n or (n and (label.min() < 0 or label.max() >= nparts)):
        raise ValueError("labels outside [0, nparts)")
    if (np.bincount(label, minlength=nparts) == 0).any():
        raise ValueError("an empty part")
    info = [0, 0, 0, 0] if info is None else info
    info[:] = [0, 0, 0, 0]
    g = _Graph(n, xadj, adj)
    prio = priority(n, seed)
    floor = max(int(min_size), 1)
    while info[0] < rounds:
        label, st = refine_round(g, label, nparts, prio, int(max_size), floor)
        if hook is not None:
            hook(label.copy(), st)
        if not st["candidates"]:
            info[3] = 1
            break
        info[0] += 1
        info[1] += st["movers"]
        info[2] += st["gain"]
    return label.astype(np.int32)


def edge_cut(n, xadj, adj, part):
    """Edges (u, v), u < v, whose ends lie in different parts."""
    g = _Graph(n, xadj, adj)
    p = np.asarray(part, np.int64)
    return int(((p[g.src] != p[g.dst]) & (g.src < g.dst)).sum())


def partition_graph(n, xadj, adj, elems_per_agg, min_shared=1, lloyd_iters=DEFAULT_LLOYD_ITERS, max_size=-1,
                    min_size=-1, seed=0, seeding=0, growth=0, growth_info=None, balanced_hook=None, refine_rounds=0, refine_info=None, refine_hook=None):
    """One level: symmetric CSR graph -> (part int32 (n), nparts).  min_shared is not used here (graph given).
    growth_info: a list that receives the four counts of the last growth (zeros for growth = 0).  balanced_hook(label,
    nlabels) is called after every balanced phase, before its release (unlabelled nodes are -1).  refine_rounds > 0: the
    refinement pass (`refine_graph`) after the merges, with the resolved caps; refine_info receives its four counts."""
    if elems_per_agg < 1 or n < 0:
        raise ValueError("elems_per_agg >= 1 and n >= 0")
    if seeding not in (0, 1):
        raise ValueError("seeding: 0 or 1")
    if growth not in (0, 1):
        raise ValueError("growth: 0 or 1")
    info = [0, 0, 0, 0] if growth_info is None else growth_info
    info[:] = [0, 0, 0, 0]
    if n == 0:
        return np.zeros(0, np.int32), 0
    max_size, min_size = resolve_sizes(elems_per_agg, max_size, min_size)
    g = _Graph(n, xadj, adj)
    prio = priority(n, seed)
    target = -(-n // elems_per_agg)
    isseed = np.zeros(n, bool)
    if seeding == 0:
        label, nlabels = _reseed(g, np.zeros(n, np.int64), isseed, prio, 1, np.array([target], np.int64))
    else:
        seeds = spaced_seeds(g, prio, target)["seeds"]
        seeds = seeds[np.argsort(prio[seeds], kind="stable")]
        label, nlabels = np.full(n, -1, np.int64), len(seeds)
        label[seeds] = np.arange(nlabels)
        isseed[seeds] = True
    def grow(label, nlabels):
        if growth == 1:
            return _grow_balanced(g, label, isseed, prio, nlabels, elems_per_agg, info, balanced_hook)
        return _grow(g, label, isseed, prio, nlabels)

    label, nlabels = grow(label, nlabels)
    for _ in range(lloyd_iters):
        label = _recentre(g, label, isseed, prio, nlabels)
        label, nlabels = grow(label, nlabels)
    if max_size > 0:
        for _ in range(REPAIR_ROUNDS):
            sizes = np.bincount(label, minlength=nlabels)
            over = sizes > max_size
            if not over.any():
                break
            k = np.where(over, np.maximum(2, -(-sizes // elems_per_agg)), 0)
            old = label
            label, nlabels = _reseed(g, label, isseed, prio, nlabels, k)
            label, nlabels = _grow(g, label, isseed, prio, nlabels, dom=old)
    if min_size > 0:
        for _ in range(MERGE_ROUNDS):
            label, moved = _merge_round(g, label, nlabels, max_size, min_size)
            if not moved:
                break
    if refine_info is not None:
        refine_info[:] = [0, 0, 0, 0]
    if refine_rounds:
        label, nlabels = renumber(label, nlabels)      # (merged labels leave holes; the pass wants every label in use)
        label = refine_graph(n, xadj, adj, label, nlabels, refine_rounds, max_size, min_size, seed, refine_info, refine_hook)
    return renumber(label, nlabels)


def quotient_graph(n, xadj, adj, part, nparts):
    g = _Graph(n, xadj, adj)
    p, q = np.asarray(part, np.int64)[g.src], np.asarray(part, np.int64)[g.dst]
    cut = p != q
    k = np.unique(p[cut] * nparts + q[cut])
    xq = np.concatenate([[0], np.cumsum(np.bincount(k // nparts, minlength=nparts))]).astype(np.int64)
    return xq, (k % nparts).astype(np.int32)


def partition_mesh(elem_ptr, elem_to_dof, ND, elems_per_agg, **opts):
    """All levels: elems_per_agg is a sequence, one entry per coarsening, and so is refine_rounds when given (the quotient
    graphs are those of the refined partitions).  Returns (parts, nparts, graphs): graphs[k] is the
    (xadj, adj) that parts[k] partitions, graphs[len(parts)] the quotient graph of the last level."""
    min_shared = opts.get("min_shared", 1)
    graphs = [build_element_graph(elem_ptr, elem_to_dof, ND, min_shared)]
    parts, nparts = [], []
    n = len(elem_ptr) - 1
    opts = dict(opts)
    refine_rounds = opts.pop("refine_rounds", None)      # one count per coarsening; refine_info: the last level's
    for k, epa in enumerate(elems_per_agg):
        xadj, adj = graphs[-1]
        if refine_rounds is not None:
            opts["refine_rounds"] = int(refine_rounds[k])
        part, npt = partition_graph(n, xadj, adj, int(epa), **opts)
        parts.append(part)
        nparts.append(npt)
        graphs.append(quotient_graph(n, xadj, adj, part, npt))
        n = npt
    return parts, nparts, graphs


def size_stats(part, nparts, elems_per_agg):
    s = np.bincount(part, minlength=nparts) / float(elems_per_agg)
    return dict(min=float(s.min()), median=float(np.median(s)), p95=float(np.percentile(s, 95)), max=float(s.max()))

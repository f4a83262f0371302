"""Agglomerates for the tests of the local order of the agglomerate matrices (saamge_amd/ae_order_model.py): a case is
(dofs, elems) -- the agglomerate's global dof numbers in table order and the dof lists of its elements.

The four agglomerates of DESIGN's table are sets of lattice points with 27-point coupling: the elements are the unit cubes
of the lattice, each with the corners that lie in the set (1 .. 8 dofs).  Their global numbers come from one of three
numberings of a G x G x G lattice of vertices: lexicographic, a coarse-vertices-first numbering in the manner of uniform
refinement (the vertices whose coordinates are all multiples of 8 first, then those of 4, of 2, the rest; lexicographic
inside a class), and a fixed random permutation."""
import numpy as np

G = 24
NUMBERINGS = ("lexicographic", "refinement", "random")


def _numbering(kind):
    k, j, i = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    lex = (i + G * (j + G * k)).ravel()
    if kind == "lexicographic":
        return lex.reshape(G, G, G)
    if kind == "refinement":
        cls = np.full(G ** 3, 3)
        for c, m in ((2, 2), (1, 4), (0, 8)):
            cls[((i % m == 0) & (j % m == 0) & (k % m == 0)).ravel()] = c
        order = np.lexsort((lex, cls))
    else:       # "random" (the fixed one of the table) or ("random", seed)
        order = np.random.RandomState(20240607 if kind == "random" else kind[1]).permutation(G ** 3)
    num = np.empty(G ** 3, np.int64)
    num[order] = np.arange(G ** 3)
    return num.reshape(G, G, G)       # [k, j, i]


_num = {}


def lattice_case(points, kind, shift=(0, 0, 0)):
    """points: iterable of (i, j, k) >= 0; the unit cubes with the corners that lie in the set"""
    if kind not in _num:
        _num[kind] = _numbering(kind)
    num = _num[kind]
    pts = {(int(i) + shift[0], int(j) + shift[1], int(k) + shift[2]) for i, j, k in points}
    gid = {p: int(num[p[2], p[1], p[0]]) for p in pts}
    elems, dofs, seen = [], [], set()
    for c in sorted({(i - a, j - b, k - d) for i, j, k in pts for a in (0, 1) for b in (0, 1) for d in (0, 1)},
                    key=lambda t: (t[2], t[1], t[0])):
        e = [gid[(c[0] + a, c[1] + b, c[2] + d)] for d in (0, 1) for b in (0, 1) for a in (0, 1)
             if (c[0] + a, c[1] + b, c[2] + d) in gid]
        if e:
            elems.append(e)
            for g in e:
                if g not in seen:
                    seen.add(g)
                    dofs.append(g)
    return np.array(dofs, np.int64), elems


def box_points(a, b, c):
    return [(i, j, k) for k in range(c) for j in range(b) for i in range(a)]


def ball_points(r):
    return [(i + r, j + r, k + r) for k in range(-r, r + 1) for j in range(-r, r + 1) for i in range(-r, r + 1)
            if i * i + j * j + k * k <= r * r]


def plate_points():
    return [(i, j, k) for k in range(4) for j in range(12) for i in range(12) if not (i >= 6 and j >= 6)]


TABLE = {       # name: (points, rows)
    "box_9x9x5": (box_points(9, 9, 5), 405),
    "box_5x5x3": (box_points(5, 5, 3), 75),
    "ball_r5": (ball_points(5), 515),
    "plate_L_4": (plate_points(), 432),
}


def table_case(name, kind, shift=(0, 0, 0)):
    dofs, elems = lattice_case(TABLE[name][0], kind, shift)
    assert len(dofs) == TABLE[name][1]
    return dofs, elems


def _first_seen(elems):
    seen, dofs = set(), []
    for e in elems:
        for g in e:
            if g not in seen:
                seen.add(g)
                dofs.append(g)
    return np.array(dofs, np.int64), [list(e) for e in elems]


def single_dof():
    return _first_seen([[7]])


def two_components_and_isolated():
    # a 8 x 8 patch of quads, a chain of 30 triangles, and a one-dof element; the three sets of numbers interleaved and scrambled
    q = np.random.RandomState(2).permutation(81) * 3
    t = np.random.RandomState(9).permutation(32) * 3 + 1
    quads = [[int(q[i + 9 * j]), int(q[i + 1 + 9 * j]), int(q[i + 9 * (j + 1)]), int(q[i + 1 + 9 * (j + 1)])] for j in range(8) for i in range(8)]
    tris = [[int(t[k]), int(t[k + 1]), int(t[k + 2])] for k in range(30)]
    return _first_seen(quads + tris + [[2]])


def path(n=80):
    ids = np.random.RandomState(3).permutation(n) * 2 + 1
    return _first_seen([[int(ids[i]), int(ids[i + 1])] for i in range(n - 1)])


def star(n=150):
    ids = np.random.RandomState(4).permutation(n + 1)
    return _first_seen([[int(ids[0]), int(ids[i])] for i in range(1, n + 1)])


def wide_level(n=300):
    # a hub (the smallest number) joined to every node of a chain whose numbers are scrambled: from an end of the chain
    # the second level holds n - 2 nodes
    ids = np.random.RandomState(5).permutation(n) + 1
    return _first_seen([[0, int(ids[i]), int(ids[i + 1])] for i in range(n - 1)])


def mixed_sizes():
    # a 12 x 8 sheet of quads with every third quad cut into two triangles, plus edge elements along one side; random numbers
    ids = np.random.RandomState(6).permutation(13 * 9)
    v = lambda i, j: int(ids[i + 13 * j])
    elems = []
    for j in range(8):
        for i in range(12):
            if (i + j) % 3 == 0:
                elems += [[v(i, j), v(i + 1, j), v(i + 1, j + 1)], [v(i, j), v(i + 1, j + 1), v(i, j + 1)]]
            else:
                elems.append([v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)])
    elems += [[v(i, 0), v(i + 1, 0)] for i in range(12)]
    return _first_seen(elems)


def coarse_pair():
    # two elements of 30 dofs each sharing 10: the shape of a coarse-level agglomerate (cliques); numbers spread out
    ids = np.random.RandomState(7).permutation(50) * 5
    return _first_seen([[int(x) for x in ids[:30]], [int(x) for x in ids[20:]]])


def coarse_chain(m=12):
    # m elements of 30 dofs, consecutive ones sharing 10, random numbers: 20 m + 10 rows
    ids = np.random.RandomState(8).permutation(20 * m + 10)
    return _first_seen([[int(x) for x in ids[20 * q:20 * q + 30]] for q in range(m)])


SMALL = {
    "single_dof": single_dof,
    "two_components_and_isolated": two_components_and_isolated,
    "path": path,
    "star": star,
    "wide_level": wide_level,
    "mixed_sizes": mixed_sizes,
    "coarse_pair": coarse_pair,
    "coarse_chain": coarse_chain,
    "box_left_alone": lambda: table_case("box_5x5x3", "lexicographic"),
    "rows_over_256": lambda: table_case("box_9x9x5", "random"),
}


def big_box():
    """13 x 13 x 8 vertices under the random numbering: 1352 rows, more than a bit matrix in LDS holds"""
    return lattice_case(box_points(13, 13, 8), "random")


def all_cases():
    """name -> (dofs, elems): the small cases and the four agglomerates of the table under the three numberings"""
    out = {k: f() for k, f in SMALL.items()}
    for name in TABLE:
        for kind in NUMBERINGS:
            out["%s/%s" % (name, kind)] = table_case(name, kind)
    return out


def mesh_of_cases(cases):
    """One mesh holding every case as an agglomerate of its own: the numbers of a case are compacted (their order kept)
    and shifted behind the cases before it.  Returns (ND, elem_ptr, elem_to_dof, part, names)."""
    ep, e2d, part, names, base = [0], [], [], [], 0
    for p, (name, (dofs, elems)) in enumerate(cases.items()):
        u = np.unique(dofs)
        for e in elems:
            e2d += [base + int(x) for x in np.searchsorted(u, e)]
            ep.append(len(e2d))
            part.append(p)
        base += len(u)
        names.append(name)
    return base, np.array(ep, np.int32), np.array(e2d, np.int32), np.array(part, np.int32), names

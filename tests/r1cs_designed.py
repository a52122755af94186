"""A constraint system with DESIGNED values for the witness map and the QAP column sums, and its model (TEST INFRASTRUCTURE: plain
Python integers, no GPU, no oracle).

k_r1cs_evaluate (csrc/mnt753_r1cs.hip), k_qap_chunks and k_qap_fold (csrc/qap_kernels.hip.h) share one piece of lazy arithmetic: a
coefficient in the device radix (c R', R' = 2^756) times an operand as it lies in wire form (x R mod r, R = 2^768), products added
limb-wise without carries, one fp_norm per two terms behind a `pending` counter, a flush and one fp_canon at the end.  Every other input
the suite feeds them is uniform, so no sum is = 0 (mod r), no operand sits at the edge of its range and the short rows, where `pending`
ends on 0 or on 1, meet random values only.  The families here plant those cases.

Designed field elements are chosen by what the kernel sees: for a wanted WIRE integer X the element is X R^-1 mod r (`elements`).
r - 4096 is among the wire integers because R / R' = 2^12 and r = 1 (mod 2^12): the device form of that coefficient is = r - 1, where
the wire integer r - 1 has a tiny device form (about r / 4096).

Witness map (`designed_system`, `shapes`, `satisfied_system`): rows as lists of (variable, coefficient); the same row set goes into a, b
and c, rotated; the model is `evaluate`.  QAP (`qap_system`): columns designed around the chunk size L and the Lagrange values u;
the model `qap_model` sums by chunk and then folds, the way the device does, and asserts which partial sums are zero and which are not.
The builders assert that every class they promise is present, so that a later edit cannot empty one silently;
tests/test_r1cs_designed_cpu.py pins the models to the oracle and to qap_ref.instance_map, tests/test_r1cs_designed_gpu.py runs the
kernels on all of it.
"""
import collections
import random

import numpy as np

import domain_ref as D

System = collections.namedtuple("System", "curve num_inputs m nc rows w")            # rows: [a, b, c], a matrix a list of rows
QapSystem = collections.namedtuple("QapSystem", "curve num_inputs m nc rows classes L")
CHAIN_LENGTHS = (1, 2, 3, 4, 5, 200, 201)
WAVE = 64
BLOCK_ROWS = 70


# ---- designed elements --------------------------------------------------------------------------------------------------------------
def wire_targets(curve):
    """(name, wire integer) the kernels are to see"""
    r = D.MODULUS[curve]
    out = [("0", 0), ("1", 1), ("r-1", r - 1), ("r-2", r - 2), ("r/2", r // 2), ("r/2+1", r // 2 + 1), ("2^752", 1 << 752),
           ("limb", (1 << 28) - 1), ("26limbs", (1 << (28 * 26)) - 1), ("2^753-1", ((1 << 753) - 1) % r), ("r-4096", r - 4096)]
    assert all(0 <= x < r for _, x in out) and len({x for _, x in out}) == len(out)
    assert r % 4096 == 1 and (r - 4096) * pow(4096, -1, r) % r == r - 1            # the device form of wire r - 4096 is = r - 1
    return out


def elements(curve):
    """the designed field elements: one per wanted wire integer, then the plain 1, 2 and r - 1"""
    r = D.MODULUS[curve]
    rinv = pow(D.R, -1, r)
    out = [x * rinv % r for _, x in wire_targets(curve)] + [1, 2, r - 1]
    assert [v * D.R % r for v in out[:-3]] == [x for _, x in wire_targets(curve)]
    assert len(set(out)) == len(out)
    return out


def largest_pair(curve):
    """(coefficient, variable value): the coefficient whose device form is = r - 1 with the operand whose wire integer is r - 1"""
    e = elements(curve)
    names = [n for n, _ in wire_targets(curve)]
    return e[names.index("r-4096")], e[names.index("r-1")]


# ---- the witness map ----------------------------------------------------------------------------------------------------------------
def csr(curve, rows):
    """rows -> (row_ptr u64 [nc + 1], col u32 [nnz], coeff wire words u64 [nnz, 12])"""
    rp = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        rp[1:] = np.cumsum([len(row) for row in rows])
    col = np.array([k for row in rows for k, _ in row], dtype=np.uint32)
    cf = D.to_wire(curve, [c for row in rows for _, c in row]) if col.size else np.zeros((0, 12), dtype=np.uint64)
    return rp, col, cf


def matrices(system):
    return [csr(system.curve, rows) for rows in system.rows]


def matrices_int(system):
    """the matrices as qap_ref.instance_map takes them: the coefficients back from the wire words as integers"""
    return [(rp, col, D.from_wire(system.curve, cf) if col.size else []) for rp, col, cf in matrices(system)]


def witness_words(system):
    return D.to_wire(system.curve, system.w)


def row_sums(system):
    r = D.MODULUS[system.curve]
    return [[sum(c * system.w[k] for k, c in row) % r for row in rows] for rows in system.rows]


def evaluate(system, out_len):
    """the model of mnt753_r1cs_evaluate: ca, cb, cc as integers, out_len entries each (r1cs_to_qap.tcc:223-237 in words: the rows,
    then (1, w)[0 .. num_inputs] in ca, zero everywhere else)"""
    assert out_len >= system.nc + system.num_inputs + 1
    out = []
    for which, sums in enumerate(row_sums(system)):
        tail = list(system.w[:system.num_inputs + 1]) if which == 0 else []
        out.append(sums + tail + [0] * (out_len - system.nc - len(tail)))
    return out


def evaluate_words(system, out_len):
    return [D.to_wire(system.curve, v) for v in evaluate(system, out_len)]


def work_waves(rows3):
    """the row lengths of every wave of 64 work items: the rows of the three matrices by decreasing length, as mnt753_r1cs_create
    orders them (a stable counting sort over (matrix, row))"""
    lens = sorted((len(row) for rows in rows3 for row in rows), reverse=True)
    return [lens[i:i + WAVE] for i in range(0, len(lens), WAVE)]


def _rotate(rows, by):
    """the interior rows rotated; the first and the last row stay, so that every matrix begins and ends with the same (empty) rows"""
    inner = rows[1:-1]
    by %= len(inner)
    return [rows[0]] + inner[by:] + inner[:by] + [rows[-1]]


def designed_rows(curve):
    """-> (rows, w, info): one matrix's rows over the assignment w = (1, designed elements); info names the classes (row indices)"""
    r = D.MODULUS[curve]
    el = elements(curve)
    w = [1] + el
    nv = len(w)
    rng = random.Random(4753 + curve)
    info = collections.defaultdict(list)
    rows = []

    def add(cls, row):
        info[cls].append(len(rows))
        rows.append(list(row))

    add("empty", [])                                                       # the first row
    for c in el:                                                           # every (coefficient, variable) pair, constant column included
        for k in range(nv):
            add("pair", [(k, c)])
    cmax, xmax = largest_pair(curve)
    kmax = w.index(xmax)
    cr1 = el[[n for n, _ in wire_targets(curve)].index("r-1")]             # wire r - 1 as the coefficient too
    for n in CHAIN_LENGTHS:                                                # both parities of `pending`, a long chain at the top of the range
        add(f"chain{n}", [(kmax, cmax)] * n)
        add(f"chain{n}", [(kmax, cr1)] * n)
    add("empty", [])
    for i, c in enumerate(el):                                             # sums that are = 0, = 1, = r - 1 (mod r)
        k = 1 + (i * 5 + 2) % (nv - 1)
        x = w[k]
        add("zero2", [(k, c), (k, (r - c) % r)])
        add("zero3", [(k, c), (k, (r - c) % r), (0, 0)])
        add("zero8", [(k, c)] * 7 + [(k, (r - 7 * c) % r)])
        add("one", [(k, c), (0, (1 - c * x) % r)])
        add("minus_one", [(k, c), (0, (r - 1 - c * x) % r)])
    add("empty", [])
    for n in (3, 2, 1, 0):                                                 # ~70 rows of each short length, random designed values
        for _ in range(BLOCK_ROWS):
            add("block", [(rng.randrange(nv), rng.choice(el)) for _ in range(n)])
            info[f"block{n}"].append(len(rows) - 1)
    add("empty", [])                                                       # the last row
    sums = [sum(c * w[k] for k, c in row) % r for row in rows]
    for cls, want in (("zero2", 0), ("zero3", 0), ("zero8", 0), ("one", 1), ("minus_one", r - 1), ("empty", 0)):
        assert info[cls] and all(sums[i] == want for i in info[cls]), cls
    for cls, n in (("zero2", 2), ("zero3", 3), ("zero8", 8)):
        assert len(info[cls]) == len(el) and all(len(rows[i]) == n for i in info[cls])
        assert sum(1 for i in info[cls] if rows[i][0][1] != 0) >= len(el) - 1       # real cancellations, not 0 + 0
    for n in CHAIN_LENGTHS:
        assert [len(rows[i]) for i in info[f"chain{n}"]] == [n, n]
    for n in (3, 2, 1, 0):
        assert len(info[f"block{n}"]) == BLOCK_ROWS and all(len(rows[i]) == n for i in info[f"block{n}"])
    assert len(info["pair"]) == len(el) * nv and rows[0] == [] and rows[-1] == []
    assert sum(1 for s in sums if s == 0) >= 3 * len(el) + 4 and len(rows) < 1200
    info["mixed_block"] = (info["block"][0], info["block"][-1] + 1)
    return rows, w, dict(info)


def designed_system(curve, num_inputs=3):
    """the full designed system: a = the rows, b and c the same rows rotated by a third and by two thirds"""
    rows, w, info = designed_rows(curve)
    nc = len(rows)
    rows3 = [rows, _rotate(rows, nc // 3), _rotate(rows, 2 * nc // 3)]
    assert rows3[0] != rows3[1] != rows3[2] != rows3[0]
    waves = work_waves(rows3)
    mixed = [wv for wv in waves if len(set(wv)) > 1]
    assert len(mixed) >= 4 and sum(1 for wv in mixed if len({n & 1 for n in wv}) == 2) >= 4, "waves of mixed length and parity"
    for n in CHAIN_LENGTHS + (8,):
        assert any(len(row) == n for row in rows)
    return System(curve, num_inputs, len(w) - 1, nc, rows3, w), info


def _with(system, **kw):
    return system._replace(**kw)


def shapes(curve):
    """-> [(name, System, out_len)]: the shapes at which the kernel's indexing can go wrong, each a cut or a variant of the designed system"""
    full, _ = designed_system(curve)
    m, nc = full.m, full.nc
    out = []
    none = _with(full, nc=0, rows=[[], [], []])
    for extra in (0, 5):
        out.append((f"nc0+{extra}", none, none.num_inputs + 1 + extra))
    chain = max(full.rows[0], key=len)
    out.append(("nc1", _with(full, nc=1, rows=[[chain], [full.rows[1][1]], [[]]]), 1 + full.num_inputs + 1))
    out.append(("inputs0", _with(full, num_inputs=0), nc + 1))
    out.append(("inputs_m", _with(full, num_inputs=m), nc + m + 1 + 2))
    out.append(("exact", full, nc + full.num_inputs + 1))
    out.append(("zero_tail", full, nc + full.num_inputs + 1 + 300))
    cut_nc = 250                                                           # 3 out_len one below, at and one above a multiple of 256
    cut = _with(full, nc=cut_nc, rows=[[rows[i * nc // cut_nc] for i in range(cut_nc)] for rows in full.rows])
    assert cut_nc + cut.num_inputs + 1 <= 255
    for out_len in (255, 256, 257):
        assert (3 * out_len) % 256 == {255: 253, 256: 0, 257: 3}[out_len]
        out.append((f"len{out_len}", cut, out_len))
    out.append(("b_empty", _with(full, rows=[full.rows[0], [[] for _ in range(nc)], full.rows[2]]), nc + full.num_inputs + 3))
    names = [n for n, _, _ in out]
    assert len(set(names)) == len(names)
    return out


def swap_system(curve):
    """a touches the variables 0 .. 2 only, b all of them: swap_ab_if_beneficial exchanges them"""
    full, _ = designed_system(curve)
    a = [[(k, c) for k, c in row if k <= 2] for row in full.rows[0]]
    sysm = _with(full, rows=[a, full.rows[1], full.rows[2]])
    touched = [len({k for row in rows for k, _ in row}) for rows in sysm.rows[:2]]
    assert touched[1] > touched[0] > 0
    return sysm


def swapped(system):
    return _with(system, rows=[system.rows[1], system.rows[0], system.rows[2]])


def satisfied_system(curve):
    """a and b designed, c one term per row on the constant column equal to ca cb: the assignment satisfies every row.  Rows with the
    products (r - 1)^2, 0 x and 1 1 are appended as pairs.  -> (System, info, the rows to disturb: 0, one in the mixed block, nc - 1)"""
    full, info = designed_system(curve)
    r = D.MODULUS[curve]
    a, b = [list(x) for x in full.rows[0]], [list(x) for x in full.rows[1]]
    base = full.rows[0]
    pairs = [(base[info["minus_one"][1]], base[info["minus_one"][2]]), (base[info["zero8"][1]], base[info["chain201"][0]]),
             (base[info["chain5"][0]], base[info["zero2"][3]]), (base[info["one"][1]], base[info["one"][4]])]
    for ra, rb in pairs:                                                   # in front of the last (empty) row
        a.insert(len(a) - 1, list(ra))
        b.insert(len(b) - 1, list(rb))
    nc = len(a)
    sysm = _with(full, nc=nc, rows=[a, b, [[] for _ in range(nc)]])
    sa, sb, _ = row_sums(sysm)
    sysm = _with(sysm, rows=[a, b, [[(0, x * y % r)] for x, y in zip(sa, sb)]])
    prods = list(zip(sa, sb))
    assert (r - 1, r - 1) in prods and (1, 1) in prods
    assert any(x == 0 and y != 0 for x, y in prods) and any(x != 0 and y == 0 for x, y in prods)
    lo, hi = info["mixed_block"]
    disturb = (0, (lo + hi) // 2, nc - 1)
    assert lo < disturb[1] < hi and a[0] == [] and a[nc - 1] == []
    return sysm, info, disturb


def disturbed(system, rows_changed):
    """c's term of the given rows raised by one: those rows are no longer satisfied"""
    r = D.MODULUS[system.curve]
    c = [list(row) for row in system.rows[2]]
    for i in rows_changed:
        c[i] = [(0, (c[i][0][1] + 1) % r)]
    return _with(system, rows=[system.rows[0], system.rows[1], c])


# ---- the QAP column sums ------------------------------------------------------------------------------------------------------------
QAP_INPUTS = 3


def qap_rows(L):
    """constraints of the designed column systems: 2 L + 2, so that a column of 2 L + 1 terms has rows to stand on"""
    return 2 * L + 2


def _columns_to_rows(nc, columns):
    rows = [[] for _ in range(nc)]
    for col in sorted(columns):
        for row, c in columns[col]:
            rows[row].append((col, c))
    return rows


def qap_system(curve, L, u=None):
    """The designed columns, for chunks of L terms.  With the Lagrange values u (every u[row] non-zero) the cancelling coefficients are
    computed from them; with u = None (t inside the domain, u an indicator vector) those places hold designed elements instead.

    Columns of a (num_inputs = 3, so columns 0 .. 3 carry the seed u[nc + i]):
        0   one term -u[nc] / u[row]: the seed cancels, At[0] = 0            1   no term: the seed alone
        2   one term per designed element, and the seed                      3   L + 1 terms that cancel the seed in the fold
        4   L + 1 terms, 5: 2 L + 1 terms: every chunk partial non-zero, their sum = 0 in the fold
        6   (row, col) repeated with c and -c: one chunk whose partial is = 0
        7   exactly L random designed terms (one full chunk)                 8 ..  one column per designed element, a single term
    b and c: the same layout with other random values; columns 0 and 1 empty, column 3 cancels without a seed."""
    r = D.MODULUS[curve]
    el = elements(curve)
    nz = [e for e in el if e]
    nc, ni = qap_rows(L), QAP_INPUTS
    rng = random.Random(7000 + 10 * L + curve)
    if u is not None:
        assert len(u) >= nc + ni + 1 and all(u[i] for i in range(nc + ni + 1))
    classes = collections.defaultdict(list)

    def cancelling(which, col, n, seed):
        """n terms on rows 0 .. n - 1, the last one -(seed + sum of the others) / u[n - 1]"""
        terms = [(row, rng.choice(nz)) for row in range(n - 1)]
        if u is None:
            return terms + [(n - 1, rng.choice(nz))]
        acc = (seed + sum(c * u[row] for row, c in terms)) % r
        classes["fold_cancel"].append((which, col))
        return terms + [(n - 1, -acc * pow(u[n - 1], -1, r) % r)]

    mats = []
    for which in range(3):
        cols = {}
        seed = (lambda i: u[nc + i] if (u is not None and which == 0) else 0)
        if which == 0:
            row0 = 5
            cols[0] = [(row0, (-u[nc] * pow(u[row0], -1, r) % r) if u is not None else rng.choice(nz))]
            classes["cancelled_seed" if u is not None else "seed_plus_term"].append((0, 0))
            classes["seed_alone"].append((0, 1))
        else:
            classes["empty"] += [(which, 0), (which, 1)]
        cols[2] = [((3 * i + which) % nc, e) for i, e in enumerate(el)]
        cols[3] = cancelling(which, 3, L + 1, seed(3))
        cols[4] = cancelling(which, 4, L + 1, 0)
        cols[5] = cancelling(which, 5, 2 * L + 1, 0)
        c = rng.choice(nz)
        cols[6] = [(7, c), (7, (r - c) % r)]
        classes["pair_cancel"].append((which, 6))
        cols[7] = [(row, rng.choice(nz)) for row in range(1, L + 1)]
        for i, e in enumerate(el):
            cols[8 + i] = [((5 * i + 2 * which + 1) % nc, e)]
        classes["designed"] += [(which, 2)] + [(which, 8 + i) for i in range(len(el))]
        classes["split"] += [(which, col) for col in cols if len(cols[col]) > L]
        mats.append(_columns_to_rows(nc, cols))
    m = 8 + len(el) - 1
    assert set(classes["split"]) >= {(k, col) for k in range(3) for col in (3, 4, 5)} and (L < len(el) or len(classes["split"]) == 9)
    assert len(classes["pair_cancel"]) == 3 and len(classes["seed_alone"]) == 1
    assert u is None or (len(classes["fold_cancel"]) == 9 and len(classes["cancelled_seed"]) == 1)
    assert all(k <= m for rows in mats for row in rows for k, _ in row)
    return QapSystem(curve, ni, m, nc, mats, dict(classes), L)


def qap_variant(qs, empty):
    """the same system with the matrices listed in `empty` left without a term"""
    rows = [[[] for _ in range(qs.nc)] if k in empty else qs.rows[k] for k in range(3)]
    return qs._replace(rows=rows)


def qap_partials(qs, u):
    """per matrix and column the partial sums of its chunks of L terms (rows ascending, repeated pairs in the order they stand), as
    qap_build_transpose cuts them"""
    r = D.MODULUS[qs.curve]
    out = []
    for rows in qs.rows:
        terms = [[] for _ in range(qs.m + 1)]
        for row, trm in enumerate(rows):
            for col, c in trm:
                terms[col].append(c * u[row] % r)
        out.append([[sum(t[i:i + qs.L]) % r for i in range(0, len(t), qs.L)] for t in terms])
    return out


def qap_model(qs, u, check_classes=True):
    """-> (At, Bt, Ct): the fold of the chunk partials and, in At, the seeds u[nc + i].  With check_classes the designed properties are
    asserted: which partial sums and which folds are = 0 and which are not."""
    r = D.MODULUS[qs.curve]
    parts = qap_partials(qs, u)
    out = []
    for which in range(3):
        v = [sum(p) % r for p in parts[which]]
        if which == 0:
            for i in range(qs.num_inputs + 1):
                v[i] = (v[i] + u[qs.nc + i]) % r
        out.append(v)
    if check_classes:
        cl = qs.classes
        for which, col in cl.get("fold_cancel", []):
            p = parts[which][col]
            assert len(p) >= 2 and all(p) and out[which][col] == 0, ("no single partial is zero, the fold is", which, col)
        for which, col in cl.get("cancelled_seed", []):
            assert out[which][col] == 0 and u[qs.nc + col] != 0 and len(parts[which][col]) == 1
        for which, col in cl["seed_alone"]:
            assert parts[which][col] == [] and out[which][col] == u[qs.nc + col] != 0
        for which, col in cl["pair_cancel"]:
            assert parts[which][col] == [0] and out[which][col] == 0 and any(qs.rows[which][7])
        for which, col in cl.get("empty", []):
            assert parts[which][col] == [] and out[which][col] == 0
        for which, col in cl["split"]:
            assert len(parts[which][col]) >= 2
    return out


def zero_columns(qs):
    """(matrix, column) whose sum the design makes = 0: these must leave the device as 24 zero words"""
    cl = qs.classes
    return sorted(set(cl.get("fold_cancel", []) + cl.get("cancelled_seed", []) + cl["pair_cancel"] + cl.get("empty", [])))


def indicator(dm, j):
    return [1 if i == j else 0 for i in range(dm)]


def row_coefficients(qs, j):
    """what At, Bt, Ct must be for t the j-th domain element: the sum of row j's coefficients per column, and 1 in column i of At for
    j = nc + i, i <= num_inputs; zero everywhere else"""
    r = D.MODULUS[qs.curve]
    out = [[0] * (qs.m + 1) for _ in range(3)]
    if j < qs.nc:
        for which in range(3):
            for col, c in qs.rows[which][j]:
                out[which][col] = (out[which][col] + c) % r
    elif j <= qs.nc + qs.num_inputs:
        out[0][j - qs.nc] = 1
    return out


def inside_indices(qs, dm):
    """j < nc in the first, second and third chunk of the long columns, j = nc + i at both ends of the inputs, j beyond both"""
    out = sorted({0, 7, qs.L, 2 * qs.L, qs.nc, qs.nc + qs.num_inputs, qs.nc + qs.num_inputs + 1, dm - 1})
    assert 2 * qs.L < qs.nc and qs.nc + qs.num_inputs + 1 <= dm - 1 and len(out) >= 7
    return out

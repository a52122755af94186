"""Model of the input tables of a verification key (TEST INFRASTRUCTURE): the plan arithmetic of
csrc/vk_input_plan.hpp in Python integers -- the table index of a digit, the bytes of the tables, the default width, the split of a
proof's inputs into slices -- and the construction of keys with many public inputs from a committed key with one.

Widened keys.  From a key (ABC_0, ABC_1) with one input x and a proof it accepts: pick a_1 .. a_k in Fr, set ABC'_j = a_j ABC_1, pick
x_1 .. x_(k-1) and solve x_k = (x - sum_{j<k} x_j a_j) / a_k mod r.  Then ABC_0 + sum_j x_j ABC'_j = ABC_0 + x ABC_1: the committed
proof verifies against the widened key with the inputs (x_1 .. x_k), and a wrong base index changes the sum."""
import pyref

SCALAR_BITS = 753
ROW_BYTES = 256
PARTIAL_BYTES = 336
TARGET_LANES = 65536
MIN_W, MAX_W = 2, 16
DEFAULT_CAP = 256 << 20


def windows(w):
    return (SCALAR_BITS + 1 + w - 1) // w


def rows_per_window(w):
    return 1 << (w - 1)


def table_bytes(points, w):
    return points * windows(w) * rows_per_window(w) * ROW_BYTES


def default_window_bits(points, cap=DEFAULT_CAP):
    """the widest w in 2 .. 16 whose tables fit cap bytes and a 32-bit row index; 0: none"""
    best = 0
    for w in range(MIN_W, MAX_W + 1):
        if table_bytes(points, w) <= cap and points * windows(w) * rows_per_window(w) < (1 << 32):
            best = w
    return best


def digit(s, j, w):
    """signed digit j of the integer s at width w (fb_digit): |d| <= 2^(w-1), sum_j d_j 2^(jw) = s"""
    win = (s >> (j * w)) & ((1 << w) - 1)
    below = (s >> (j * w - 1)) & 1 if j else 0
    top = (win >> (w - 1)) & 1
    return win + below - (top << w)


def row_of(base, j, d, w):
    """(row, negate) of digit d != 0 of window j of base `base`: window base W + j of one long table"""
    return (base * windows(w) + j) * rows_per_window(w) + abs(d) - 1, d < 0


def base_rows(base, w):
    """the rows [first, end) of the tables that belong to `base`"""
    per = windows(w) * rows_per_window(w)
    return base * per, (base + 1) * per


def inputs_per_lane(n, k):
    if k == 0:
        return 1
    want = max(1, TARGET_LANES // max(n, 1))
    s = min(want, k)
    return (k + s - 1) // s


def slices(k, ipl):
    """[(first, end)] of the scalars of one proof: ceil(k / ipl) slices, the last one may be ragged"""
    return [(a, min(k, a + ipl)) for a in range(0, k, ipl)]


def workspace_per_proof(k, ipl):
    return PARTIAL_BYTES * (len(slices(k, ipl)) + 1) + 112


# ---- widened keys ------------------------------------------------------------------------------------------------------------------
def ratios(r, k, seed):
    """a_1 .. a_k: non-zero, distinct"""
    rng = pyref.splitmix64(seed)
    out = []
    while len(out) < k:
        a = pyref.rand_below(rng, r - 1) + 1
        if a not in out:
            out.append(a)
    return out


def solve_last(r, a, xs, x):
    """x_k with sum_j x_j a_j = x mod r, given x_1 .. x_(k-1)"""
    k = len(a)
    assert len(xs) == k - 1
    rest = sum(xj * aj for xj, aj in zip(xs, a)) % r
    return (x - rest) * pow(a[k - 1], -1, r) % r


def combined(r, a, xs):
    return sum(xj * aj for xj, aj in zip(xs, a)) % r


def designed_rows(r, a, x, wrap):
    """Rows of k inputs that all combine to x (so the committed proof stays valid), k = len(a): the ends of the field, the wrap
    family (equal points meet inside one walk), two inputs whose partial sums are equal and two whose partial sums are opposite
    (k >= 3).  -> [(label, [x_1 .. x_k])]"""
    k = len(a)
    rows = []

    def close(label, head):
        head = [h % r for h in head][:k - 1]
        head += [0] * (k - 1 - len(head))
        rows.append((label, head + [solve_last(r, a, head, x)]))

    close("ends", [0, 1, r - 1] * k)
    close("ends shifted", [r - 1, 0, 1] * k)
    close("wrap", [s for _, s in wrap] * (k // max(len(wrap), 1) + 1))
    if k >= 3:
        x1 = 0x1234567 + k
        x2 = x1 * a[0] * pow(a[1], -1, r) % r
        close("equal partials", [x1, x2] + [7] * k)                   # x_1 a_1 = x_2 a_2
        close("opposite partials", [x1, r - x2] + [7] * k)            # x_1 a_1 = -x_2 a_2
    return rows

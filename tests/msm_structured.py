"""Structured scalars of the MSM's digit extraction and the reference recoding they are built around (TEST INFRASTRUCTURE).

The MSM turns every 753-bit scalar into W = ceil(754 / c) signed window digits (Booth, radix 2^c):

    d_w = s[wc .. wc+c) + s[wc-1] - 2^c s[wc+c-1]          |d_w| <= 2^(c-1),   sum_w d_w 2^(wc) = s

and the product holds three copies of that recoding (k_scalar_digits over lds_bits, k_part_pass over booth_digit, k_part_pass_c over
reg_bits<C> for C = 14 .. 22), all behind fp_wire_to_integer.  A uniform scalar gives the largest magnitude 2^(c-1) -- the last
bucket of a set, the last key of a partition, the heaviest bucket of the reduction -- with probability 2^-c per window, and almost
never a window that holds nothing but a carry.  The families here give those digits by construction, at every window of every width.

`booth` is the recoding on Python integers; it shares nothing with the device code but the definition above.  Every family is a list
of integers in [0, r) of the curve's scalar field; `wire` turns a list into the ABI's uint64 [n, 12] (Montgomery form, R = 2^768).
"""
import domain_ref as D

SCALAR_BITS = 753
WIDTHS = tuple(range(2, 23))                  # every width mnt753_msm_set_window_bits accepts


def modulus(curve):
    return D.MODULUS[curve]


def windows(c):
    """W = ceil(754 / c): one bit more than the scalar has, so that the carry of the last full window has a digit to land in"""
    return (754 + c - 1) // c


def booth(s, c):
    """the W signed digits of s (0 <= s < 2^753) at width c, lowest window first"""
    mask = (1 << c) - 1
    out = []
    for w in range(windows(c)):
        pos = w * c
        win = (s >> pos) & mask
        blo = (s >> (pos - 1)) & 1 if w else 0
        out.append(win + blo - ((win >> (c - 1)) << c))
    return out


def unbooth(digits, c):
    """sum_w d_w 2^(wc)"""
    return sum(d << (w * c) for w, d in enumerate(digits))


def coverage(ints, c):
    """{(window, digit)}: every non-zero digit the list produces at width c"""
    out = set()
    for s in ints:
        out.update((w, d) for w, d in enumerate(booth(s, c)) if d)
    return out


def top_digit_max(curve, c):
    """The largest digit the top window W - 1 can hold for a scalar below r: bit W c - 1 >= 753 is never set, so the digit is
    (s >> t) + s[t-1] with t = (W - 1) c, which grows with s; r - 1 has it (r is odd: r - 1 and r share every bit above bit 0)."""
    return booth(modulus(curve) - 1, c)[-1]


def _below_r(curve, ints):
    r = modulus(curve)
    seen, out = set(), []
    for v in ints:
        if 0 <= v < r and v not in seen:
            seen.add(v)
            out.append(v)
    return out


# ---- the families ---------------------------------------------------------------------------------------------------------------------
def single_bits(curve):
    """2^k for every bit position of a scalar: every straddle of a 32-bit word by a window, every window of every width (bit 752 is
    the top bit of r: all 753 values are below r)"""
    return _below_r(curve, [1 << k for k in range(SCALAR_BITS)])


def extremes(curve, c):
    """For every window w: 2^(wc+c-1) -- the window's top bit alone: d_w = -2^(c-1), d_(w+1) = +1 -- and for w >= 1
    2^(wc+c-1) - 2^(wc-1) -- bits wc-1 .. wc+c-2: d_w = +2^(c-1) (all ones below the top bit, plus the bit below the window) and
    d_(w-1) = -2^(c-1).  Values of r and above are left out (top windows only)."""
    out = []
    for w in range(windows(c)):
        hi = w * c + c - 1
        out.append(1 << hi)
        if w:
            out.append((1 << hi) - (1 << (w * c - 1)))
    return _below_r(curve, out)


CARRY_BITS = (31, 32, 33, 63, 64, 65, 735, 736, 737, 752)


def carry_chains(curve, c):
    """2^k - 1: -1 at window 0, zeros, and +1 (or 2^j) far above.  k: the multiples of c, where the ones end exactly at a window's
    edge, and the edges of the 32- and 64-bit words at both ends of the scalar"""
    ks = list(range(c, SCALAR_BITS, c)) + list(CARRY_BITS)
    return _below_r(curve, [(1 << k) - 1 for k in ks])


EDGE_BITS = (1, 31, 32, 64, 383, 384, 736, 751, 752)


def edges(curve):
    """the ends of the scalar field and of the 753-bit range, and the two alternating bit patterns"""
    r = modulus(curve)
    fives = int("5" * 192, 16)                # 768 bits of 01 / 10
    out = [r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, 1 << 752, (1 << 752) - 1]
    out += [r - (1 << k) for k in EDGE_BITS]
    out += [fives % r, (fives << 1) % r, 2, 3]
    return _below_r(curve, out)


def dense(curve, c):
    """1 .. 2^(c-1), then r - 1 .. r - 2^(c-1).  The first half puts one entry into every bucket of window 0: positive ones, and
    -2^(c-1) (with +1 above) for 2^(c-1) itself.  The low 15 bits of r are 0 .. 01 on both curves, so for c <= 15 the digit of r - j at
    window 0 is 1 - j: one negative entry in every bucket but the last (and nothing for j = 1); the r - j half also fills the windows
    above with the bits of r."""
    r, h = modulus(curve), 1 << (c - 1)
    return list(range(1, h + 1)) + [r - j for j in range(1, h + 1)]


FAMILIES = {"single_bits": lambda curve, c: single_bits(curve), "extremes": extremes, "carry_chains": carry_chains,
            "edges": lambda curve, c: edges(curve), "dense": dense}


def family(curve, name, c):
    return FAMILIES[name](curve, c)


def label(name, c):
    """the name a failure reports: families that depend on the width carry it"""
    return f"{name}({c})" if name in ("extremes", "carry_chains", "dense") else name


def wire(curve, ints):
    """the ABI's scalars: uint64 [n, 12], Montgomery form"""
    return D.to_wire(curve, ints)

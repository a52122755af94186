"""Designed bucket occupancies for the MSM's bucket stages, and a host model of what those stages do with them (TEST INFRASTRUCTURE).

Everything behind the MSM's sort is driven by how many entries each bucket holds: the accumulate walk (k_bucket_accumulate: lane t owns
sorted entries [tT, (t+1)T); a run that ends inside the segment is a whole bucket, the first and last run are edge pieces, a lane with one
run writes an identity as its second piece, empty keys are stepped over), the regular slot tree of the batched-affine levels
(k_pair_level: every bucket padded to a multiple of 2^L with empty entries, slots ADD / DBL / CANCEL / SINGLE / EMPTY), the irregular
levels (ceil(g / 2) slots per bucket), the edge-merge tree (one node per lane boundary a bucket crosses) and k_pair_fix.  Uniform scalars
give Poisson-sized buckets (0 .. 3 entries at test sizes) and the skewed inputs of tests/test_msm_gpu.py one giant bucket; the profiles
here place chosen counts on chosen keys instead:

    wide   g bases with the scalar j (1 <= j < 2^(c-1)): g entries in bucket j, g distinct points, all rows of window 0
    tall   one base with the scalar j * sum_{w<g} 2^(wc) (g <= W - 2): g entries in bucket j, rows of g table levels (window table only:
           one bucket set shared by all windows, key |d| - 1; without it the key is w nb + |d| - 1 and j 2^(wc) reaches set w)
    2^(c-1)  has d_0 = -2^(c-1), d_1 = +1: a negated entry in the last bucket of the set (and a carry in bucket 1 of the window above)

Which slot of a bucket an entry lands in is up to the sort stage (the atomic sort fixes no order), so every profile means the same under
any order inside a bucket: counts, "every entry of the bucket is the same point", "k copies of {P, -P}".

A profile is a function of (curve, c, ...) and returns a Profile: the scalars as integers, the base recipe (None: base k is synthetic
base k; otherwise one item per base -- ("synth",) the synthetic base of that index, ("copy", k) / ("neg", k) the point of index k or its
negative, ("gen", +1 / -1) the group generator G or -G, the stand-in point the levels write for a cancelled pair), and the designed
counts {(window, bucket number |d|): entries}, written down from the construction, not computed from the scalars.

The model restates the plan (plan_T), the slot counts the levels leave (slots), and counts the events a list of bucket sizes produces
in the accumulate walk (lane_events) and in the regular tree (tree_events).  It shares only definitions with the product.
tests/test_msm_occupancy_cpu.py checks the profiles against the reference recoding (msm_structured.booth) and that the cases listed at
the bottom -- the one list tests/test_msm_occupancy_gpu.py runs -- produce every event; the GPU file runs them.
"""
import bisect
import collections
import random

import msm_structured as S

Profile = collections.namedtuple("Profile", "ints recipe designed")

MACHINE_LANES = {1: 65536, 2: 32768, 3: 21504}   # logical lanes of one round of the chip at 1, 2, 3 threads per point


def lanes_per_point(curve, group):
    return 1 if group == 1 else (2 if curve == 0 else 3)


# ---- building blocks ------------------------------------------------------------------------------------------------------------------
def tall_scalar(j, g, c, window=0):
    """digit j in windows window .. window + g - 1 and nothing else"""
    assert 1 <= j < (1 << (c - 1)) and 1 <= g and window + g <= S.windows(c) - 2
    return sum(j << ((window + w) * c) for w in range(g))


def fill(ints, designed, j, g, c, form="wide", window=0):
    """g entries into bucket j: `wide` -- g bases, rows of `window`; `tall` -- as few bases as the windows allow, rows of windows 0 .. """
    if g == 0:
        return
    if form == "wide":
        ints += [j << (window * c)] * g
        designed[(window, j)] += g
        return
    assert form == "tall" and window == 0
    top = S.windows(c) - 2
    while g:
        h = min(g, top)
        ints.append(tall_scalar(j, h, c))
        for w in range(h):
            designed[(w, j)] += 1
        g -= h


def _profile(ints, designed, recipe=None):
    return Profile(ints, recipe, {k: v for k, v in designed.items() if v})


# ---- the profiles -----------------------------------------------------------------------------------------------------------------------
def staircase(curve, c, form="wide", top=40, window=0):
    """buckets 1 .. top hold 1 .. top entries, on adjacent keys (wide: top (top + 1) / 2 bases; tall: top bases, table mode only)"""
    ints, designed = [], collections.Counter()
    for j in range(1, top + 1):
        fill(ints, designed, j, j, c, form, window)
    return _profile(ints, designed)


def powers(curve, c, kmax=7):
    """adjacent buckets of 2^k - 1, 2^k, 2^k + 1 entries for k = 1 .. kmax, wide (kmax = 7: 762 entries)"""
    ints, designed, j = [], collections.Counter(), 1
    for k in range(1, kmax + 1):
        for g in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            fill(ints, designed, j, g, c)
            j += 1
    return _profile(ints, designed)


ALIGNED_BUCKETS = 24


def aligned(curve, c, T, phase, form="wide"):
    """bucket 1: `phase` entries (0 <= phase < T; none at phase 0), buckets 2 .. 25: T q entries with q cycling through 1, 2, 3.  At
    phase 0 every bucket end is the end of a lane of T entries, at any other phase none is."""
    assert 0 <= phase < T
    ints, designed = [], collections.Counter()
    fill(ints, designed, 1, phase, c, form)
    for k in range(ALIGNED_BUCKETS):
        fill(ints, designed, 2 + k, T * (1 + k % 3), c, form)
    return _profile(ints, designed)


ENDS_HEAVY = 37


def ends(curve, c):
    """First and last key of a set heavy, thousands of empty keys between them: 37 x the scalar 1, 37 x 2^(c-1) -- d_0 = -2^(c-1), a
    negated entry in the set's last bucket, and d_1 = +1 -- and one entry in bucket 2^(c-2).  (The carries are entries too: with the
    window table they are 37 more entries of bucket 1, rows of table level 1; without it they are bucket 1 of set 1.)"""
    half = 1 << (c - 1)
    ints = [1] * ENDS_HEAVY + [half] * ENDS_HEAVY + [half >> 1]
    return _profile(ints, collections.Counter({(0, 1): ENDS_HEAVY, (0, half): ENDS_HEAVY, (1, 1): ENDS_HEAVY, (0, half >> 1): 1}))


FULL_SET_GAP = (57, 72)


def full_set(curve, c=8):
    """every bucket of the set in play at c = 8 (128 buckets): sizes cycle through 0 .. 7 -- bucket j holds (j + 3) mod 8 entries, so
    the last one, the extreme digit, holds three negated ones --, and buckets 57 .. 72 are one run of 16 empty keys"""
    half = 1 << (c - 1)
    ints, designed = [], collections.Counter()
    for j in range(1, half + 1):
        g = 0 if FULL_SET_GAP[0] <= j <= FULL_SET_GAP[1] else (j + 3) % 8
        if j < half:
            fill(ints, designed, j, g, c)
        else:
            ints += [half] * g                 # -2^(c-1) at window 0 and +1 at window 1
            designed[(0, half)] += g
            designed[(1, 1)] += g
    return _profile(ints, designed)


def nibbles(curve, c, n, seed=20260):
    """seeded scalars uniform in 0 .. 15: 15 adjacent buckets of about n / 16 entries (and n / 16 scalars that are zero) -- a witness of
    bits, nibbles and bytes in small"""
    rng = random.Random(seed)
    ints = [rng.randrange(16) for _ in range(n)]
    return _profile(ints, collections.Counter((0, v) for v in ints if v))


def collisions(curve, c):
    """Equal and opposite points inside a bucket, next to ordinary buckets (adjacent keys from 1 on).  G is the group generator: the
    point the levels write into the slot of a cancelled pair, with fix_count[bucket] D subtracted after the edge merge.
        3 ordinary | 5, 8, 13 copies of one point | 2 ordinary | 2 x {P, -P} | 5 x {P, -P} | 4 ordinary | {P, -P} + a survivor |
        4 x {P, -P} + a survivor | {P, -P, G} | {P, -P, -G} | {G, G} | {G, -G, Q} | 3 ordinary"""
    ints, recipe, designed = [], [], collections.Counter()
    state = {"j": 0}

    def bucket(items):
        """items: "new" (a fresh synthetic point), ("copy" / "neg", index into this bucket's items), ("gen", sign)"""
        state["j"] += 1
        first = len(recipe)
        for it in items:
            recipe.append(("synth",) if it == "new" else (it if it[0] == "gen" else (it[0], first + it[1])))
            ints.append(state["j"])
        designed[(0, state["j"])] += len(items)

    pair = ["new", ("neg", 0)]
    bucket(["new"] * 3)
    for g in (5, 8, 13):
        bucket(["new"] + [("copy", 0)] * (g - 1))
    bucket(["new"] * 2)
    for k in (2, 5):
        bucket(["new"] + [("neg", 0)] * k + [("copy", 0)] * (k - 1))
    bucket(["new"] * 4)
    bucket(pair + ["new"])
    bucket(["new"] + [("neg", 0)] * 4 + [("copy", 0)] * 3 + ["new"])
    bucket(pair + [("gen", 1)])
    bucket(pair + [("gen", -1)])
    bucket([("gen", 1), ("gen", 1)])
    bucket([("gen", 1), ("gen", -1), "new"])
    bucket(["new"] * 3)
    return _profile(ints, designed, recipe)


def apply_recipe(recipe, synth, gen, negate):
    """the base points of a recipe: synth -- the synthetic bases (n, affine words); gen -- G; negate(point) -> -point"""
    if recipe is None:
        return synth
    pts = synth.copy()
    for i, it in enumerate(recipe):
        if it[0] == "copy":
            pts[i] = pts[it[1]]
        elif it[0] == "neg":
            pts[i] = negate(pts[it[1]])
        elif it[0] == "gen":
            pts[i] = gen if it[1] > 0 else negate(gen)
    return pts


def moved_scalars(curve, prof):
    """the discrete-log form of a recipe: (scalars with every copy / negative moved onto its original base, mod r; coefficient of G)"""
    r = S.modulus(curve)
    out, g = [0] * len(prof.ints), 0
    for i, (s, it) in enumerate(zip(prof.ints, prof.recipe or [("synth",)] * len(prof.ints))):
        if it[0] == "synth":
            out[i] = (out[i] + s) % r
        elif it[0] == "gen":
            g = (g + it[1] * s) % r
        else:
            out[it[1]] = (out[it[1]] + (s if it[0] == "copy" else -s)) % r
    return out, g


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def n_keys(c, table):
    return (1 << (c - 1)) * (1 if table else S.windows(c))


def occupancy(ints, c, table):
    """entries per key, from the reference recoding: key = |d| - 1 with the window table, w nb + |d| - 1 without"""
    nb = 1 << (c - 1)
    counts = [0] * n_keys(c, table)
    for s in ints:
        for w, d in enumerate(S.booth(s, c)):
            if d:
                counts[(0 if table else w * nb) + abs(d) - 1] += 1
    return counts


def designed_counts(prof, c, table):
    """the same list from the counts a profile was built for"""
    nb = 1 << (c - 1)
    counts = [0] * n_keys(c, table)
    for (w, j), g in prof.designed.items():
        counts[(0 if table else w * nb) + j - 1] += g
    return counts


def plan_T(n, c, lanes, t_min):
    """entries per accumulate lane of an MSM over n points (make_plan): one round of the machine's lanes below 2^23 entries, two from
    there on, and never fewer than t_min"""
    entries = S.windows(c) * n
    target = MACHINE_LANES[lanes] * (1 if entries < (1 << 23) else 2)
    return max((entries + target - 1) // target, t_min)


BLOCKED_T = 8    # entries per lane of the accumulate behind the levels, while the list is shorter than 8 per lane


def slots(g, L, irr=0):
    """slots a bucket of g entries has left behind L regular and irr irregular levels"""
    s = (g + (1 << L) - 1) >> L
    for _ in range(irr):
        s = (s + 1) >> 1
    return s


LANE_EVENTS = ("end_on_lane_end", "spans_3_lanes", "two_whole_buckets", "single_run_lane", "starts_behind_empty_keys", "skips_empty_keys")


def lane_events(counts, T):
    """What the accumulate walk meets on a list of bucket sizes at T entries per lane:
        end_on_lane_end          non-empty buckets whose last entry is the last entry of a lane's segment (end = 0 mod T)
        spans_3_lanes            buckets with entries in three or more lanes (inner lanes hold nothing else: trees in the edge merge)
        two_whole_buckets        lanes with two or more runs that are neither their first nor their last (written to buckets[] directly)
        single_run_lane          lanes whose segment lies inside one bucket (the identity as second edge piece)
        starts_behind_empty_keys lanes whose first entry is the first of a bucket whose key follows an empty key (the binary search
                                 lands on equal offsets)
        skips_empty_keys         runs that end inside a lane in front of one or more empty keys (do { ++b; } while (next == e))"""
    ev = dict.fromkeys(LANE_EVENTS, 0)
    starts, keys, pos = [], [], 0
    for k, g in enumerate(counts):
        if g:
            starts.append(pos); keys.append(k)
            pos += g
    total = pos
    ends = starts[1:] + [total]
    for k, s, e in zip(keys, starts, ends):
        ev["end_on_lane_end"] += e % T == 0
        ev["spans_3_lanes"] += (e - 1) // T - s // T + 1 >= 3
        behind_empty = k > 0 and counts[k - 1] == 0
        if behind_empty and s % T == 0:
            ev["starts_behind_empty_keys"] += 1
        if behind_empty and s % T != 0:
            ev["skips_empty_keys"] += 1
    for lo in range(0, total, T):
        hi = min(lo + T, total)
        runs = bisect.bisect_left(starts, hi) - bisect.bisect_right(starts, lo) + 1
        ev["single_run_lane"] += runs == 1
        ev["two_whole_buckets"] += runs - 2 >= 2
    return ev


def tree_events(counts, L):
    """The regular tree over buckets padded to a multiple of 2^L: per level l = 1 .. L the slots with two occupied children (`pair`: ADD,
    DBL or CANCEL by their values), with one (`single`) and with none (`empty`: a whole group of 2^l entries that is padding); and the
    residues g mod 2^L that occur"""
    levels = [dict(pair=0, single=0, empty=0) for _ in range(L)]
    residues = set()
    for g in counts:
        if not g:
            continue
        residues.add(g % (1 << L))
        padded = slots(g, L) << L
        for l in range(1, L + 1):
            children = slots(g, l - 1)
            levels[l - 1]["pair"] += children // 2
            levels[l - 1]["single"] += children % 2
            levels[l - 1]["empty"] += (padded >> l) - (children + 1) // 2
    return dict(levels=levels, residues=residues)


# ---- the cases: ONE list, for the coverage conditions of the CPU file and the runs of the GPU file ------------------------------------
C_TABLE = 12              # MNT753_MSM_TABLE_BITS of the table-mode cases: W = 63, 2048 buckets
C_FULL_SET = 8            # W = 95, 128 buckets; the partition passes do not apply, the atomic sort runs
C_NO_TABLE = 7            # mnt753_msm_set_window_bits: W = 108 sets of 64 buckets
FAR_WINDOW = 100          # the set "far above" of the second staircase without the table
PAIRS, IRRS, TMINS = (0, 1, 2, 3, 6), (0, 1, 3), (1, 3, 4, 8)


def knob_product(pairs, irrs, tmins, **more):
    """PAIR x IRR x TMIN, the irregular levels only behind regular ones"""
    return [dict(pair=p, irr=i, tmin=t, **more) for p in pairs for i in (irrs if p else (0,)) for t in tmins]


def run_order(knobs):
    """The order a case runs its settings in on ONE base set.  Two pieces of the library's state outlive an MSM:
      * the partition sort's buffers are allocated when the workspace is (re)built -- T, or the padded list's length, changed -- under
        a setting that asks for that sort, and an MSM that asks for it without them takes the atomic sort, unreported.  So every
        setting of the partition sorts (part, generic) runs before the first atomic one: a rebuild then never happens under `atomic`
        ahead of them;
      * the level buffers grow to the worst case of the largest PAIR seen since the workspace was last rebuilt (a rebuild drops
        them), and an irregular level that does not fit in them is dropped (the last plan's irr_levels says how many ran).  So the
        settings run TMIN by TMIN -- a new T is what rebuilds the workspace -- and within one TMIN the largest PAIR first.
    replay() below restates both rules; tests/test_msm_occupancy_cpu.py proves over the whole case list that in this order every
    non-atomic setting sorts by partition and every setting runs all the irregular levels it asks for."""
    return sorted(knobs, key=lambda k: (k["sort"] == "atomic", k["tmin"], -k["pair"]))


G1_KNOBS = knob_product(PAIRS, IRRS, TMINS, sort="part")
# the other two sort stages and both forms of every edge-tree level, at two fixed settings
G1_EXTRAS = [dict(pair=p, irr=i, tmin=t, **x) for p, i, t in ((0, 0, 3), (2, 1, 8))
             for x in (dict(sort="atomic"), dict(sort="generic"), dict(sort="part", edge_flow=0), dict(sort="part", edge_flow=100000000))]
G2_KNOBS = knob_product((0, 2), (0, 2), (1, 8), sort="part")
FULL_SET_KNOBS = knob_product((0, 2), (0, 1), (1, 3, 8), sort="atomic")      # (IRR 1 on top of what is asked for)
NO_TABLE_KNOBS = knob_product((0, 2), (0, 1), (1, 4), sort="atomic")

Case = collections.namedtuple("Case", "name build knobs c table")


def _case(name, build, knobs, c=C_TABLE, table=True):
    return Case(name, build, run_order(knobs), c, table)


def g1_cases():
    """table mode at c = 12, n <= 1024 so that W n stays below the machine's lanes and T = MNT753_MSM_TMIN"""
    c = C_TABLE
    every = G1_KNOBS + G1_EXTRAS
    out = [_case("staircase_wide", lambda curve: staircase(curve, c, "wide"), every),
           _case("staircase_tall", lambda curve: staircase(curve, c, "tall"), every),
           _case("powers", lambda curve: powers(curve, c), every),
           _case("ends", lambda curve: ends(curve, c), every),
           _case("nibbles", lambda curve: nibbles(curve, c, 1024), every),
           _case("collisions", lambda curve: collisions(curve, c), every)]
    for T in TMINS:
        if T > 1:
            for phase in (0, 1, T - 1):
                out.append(_case(f"aligned_T{T}_p{phase}", lambda curve, T=T, phase=phase: aligned(curve, c, T, phase),
                                 knob_product(PAIRS, IRRS, (T,), sort="part")))
    # behind L levels a lane of the accumulate holds 8 final slots: buckets of 8 * 2^L q entries end on its lanes
    for L in PAIRS:
        if L:
            for phase in (0, 1):
                # (these run one PAIR only, on two dozen bases: a PAIR 6 setting in front of every TMIN sizes the level buffers so that three
                # irregular levels behind one regular level fit -- run_order)
                out.append(_case(f"aligned_blocked_L{L}_p{phase}", lambda curve, L=L, phase=phase: aligned(curve, c, BLOCKED_T << L, phase, "tall"),
                                 knob_product((L,), IRRS, TMINS, sort="part") + ([dict(pair=6, irr=0, tmin=t, sort="part") for t in TMINS] if L < 6 else [])))
    return out


def g2_cases(curve):
    """the lane-split kernels, every profile at its G2 size: n <= 512 (MNT4753, two lanes per point) / 336 (MNT6753, three)"""
    c = C_TABLE
    n = 512 if curve == 0 else 336
    out = [_case("staircase_wide", lambda curve: staircase(curve, c, "wide", top=20), G2_KNOBS),
           _case("staircase_tall", lambda curve: staircase(curve, c, "tall", top=20), G2_KNOBS),
           _case("powers", lambda curve: powers(curve, c, kmax=5), G2_KNOBS),
           _case("ends", lambda curve: ends(curve, c), G2_KNOBS),
           _case("nibbles", lambda curve: nibbles(curve, c, n), G2_KNOBS),
           _case("collisions", lambda curve: collisions(curve, c), G2_KNOBS)]
    for phase in (0, 1, 7):
        out.append(_case(f"aligned_T8_p{phase}", lambda curve, phase=phase: aligned(curve, c, 8, phase, "tall"), knob_product((0, 2), (0, 2), (8,), sort="part")))
    for phase in (0, 1):
        out.append(_case(f"aligned_blocked_L2_p{phase}", lambda curve, phase=phase: aligned(curve, c, BLOCKED_T << 2, phase, "tall"),
                         knob_product((2,), (0, 2), (1, 8), sort="part")))
    return out


def full_set_case():
    return _case("full_set", lambda curve: full_set(curve, C_FULL_SET), FULL_SET_KNOBS, c=C_FULL_SET)


# Steps of the staircase without the table.  The wide form needs a base per entry; 40 steps are 820 bases, and with W = 108 windows at
# c = 7 that is W n = 88560 entries for the plan, more than the machine's 65536 lanes: T would be 2 where MNT753_MSM_TMIN asks for 1,
# and the cases are to run at T = TMIN.  34 steps are 595 bases, W n = 64260.
NO_TABLE_STEPS = 34


def no_table_cases():
    c = C_NO_TABLE
    return [_case("staircase_wide_set0", lambda curve: staircase(curve, c, "wide", top=NO_TABLE_STEPS), NO_TABLE_KNOBS, c, False),
            _case(f"staircase_wide_set{FAR_WINDOW}", lambda curve: staircase(curve, c, "wide", top=NO_TABLE_STEPS, window=FAR_WINDOW), NO_TABLE_KNOBS, c, False),
            _case("ends", lambda curve: ends(curve, c), NO_TABLE_KNOBS, c, False)]


def all_cases():
    """[(curve, group, Case)]: everything tests/test_msm_occupancy_gpu.py runs"""
    out = []
    for curve in (0, 1):
        out += [(curve, 1, cs) for cs in g1_cases() + [full_set_case()] + no_table_cases()]
        out += [(curve, 2, cs) for cs in g2_cases(curve)]
    return out


def accumulate_view(counts, knob, T):
    """(list of sizes, entries per lane) the accumulate kernel walks under a knob setting: the entries at the plan's T, or behind levels
    the slots they leave at 8 per lane (every list here is shorter than 8 slots per lane of the plan)"""
    if knob["pair"] == 0:
        return counts, T
    return [slots(g, knob["pair"], knob["irr"]) for g in counts], BLOCKED_T


def pair_cap1(n, c, table, L):
    """level-1 slots of the worst case: (W n + n_buckets (2^L - 1)) / 2 (msm_host.hpp, pair_cap1)"""
    return (S.windows(c) * n + n_keys(c, table) * ((1 << L) - 1)) // 2


def irr_levels_run(n, c, table, L, irr, pair_cap, pair_buckets):
    """irregular levels pair_and_accumulate runs of the irr asked for: level k writes at most half its input plus one slot per bucket
    into one of two row buffers -- pair_cap slots, or pair_cap / 2 + pair_buckets --, and stops at the first that does not fit"""
    nbk = n_keys(c, table)
    slots_in = (2 * pair_cap1(n, c, table, L)) >> L
    for k in range(1, irr + 1):
        slots_in = slots_in // 2 + nbk
        room = pair_cap // 2 + pair_buckets if (L + k - 1) & 1 else pair_cap
        if slots_in > room or slots_in > pair_cap // 2 + pair_buckets + 64:
            return k - 1
    return irr


def partition_fits(c, table):
    """the partition passes stage a plan in LDS (msm_sort_partition_fits): up to 4096 partitions of 1024 keys, 160 KB.  W = 63 at c = 12
    fits (there both `part` and `generic` run the passes that read the width at run time: the ones by width start at c = 14); W = 95
    at c = 8 does not"""
    parts = (n_keys(c, table) + 1023) >> 10
    return parts <= 4096 and 4 * (24 * 256 + 3 * parts + 256 + 2 * 256 * S.windows(c)) <= 160 * 1024


def replay(cs, n, lanes):
    """[(knob, sorted by partition?, irregular levels run)] of a case's settings in the order given, on one base set created under
    the first: the workspace rule of ensure_ws (reused while T, the lanes and the padded list's length fit; the partition buffers
    exist if the last rebuild happened under part / generic) and the grow-only level buffers of ensure_pair_ws"""
    W, nbk = S.windows(cs.c), n_keys(cs.c, cs.table)
    ws_T, ws_cap, has_part, pair_cap, pair_buckets = None, 0, False, 0, 0
    out = []
    for step, knob in enumerate([cs.knobs[0]] + list(cs.knobs)):          # step 0: mnt753_bases_create sizes both for the first setting
        L, T = knob["pair"], plan_T(n, cs.c, lanes, knob["tmin"])
        need = W * n + nbk * ((1 << L) - 1)
        if ws_T != T or ws_cap < need:
            ws_T, ws_cap, has_part = T, need, knob["sort"] != "atomic"
            pair_cap = pair_buckets = 0                                   # free_ws drops the set's level buffers with the workspace
        if L and (pair_cap < pair_cap1(n, cs.c, cs.table, L) or pair_buckets < nbk):
            pair_cap, pair_buckets = max(pair_cap, pair_cap1(n, cs.c, cs.table, L)), max(pair_buckets, nbk)
        if step:
            out.append((knob, has_part and knob["sort"] != "atomic" and partition_fits(cs.c, cs.table), irr_levels_run(n, cs.c, cs.table, L, knob["irr"], pair_cap, pair_buckets) if L else 0))
    return out

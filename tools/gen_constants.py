#!/usr/bin/env python3
"""Derive every numeric table the HIP field layer needs from the two MNT753 primes.

Writes snark-challenge-prover-reference_amd/csrc/mnt753_constants.h, mnt753_pairing_constants.h and mnt753_sqrt_constants.h (committed; regenerate
with `python tools/gen_constants.py`).  Inputs are the decimal literals in tools/mnt753_params.py,
which cite the reference's curve-initialisation files line by line.

Internal device representation (see DESIGN.md "field layer"):
  27 limbs x 28 bits, Montgomery radix R' = 2^756, values kept in [0, 2p).
File / wire representation (libsnark/serialization.hpp:22-34 of the reference):
  12 limbs x 64 bits, Montgomery radix R = 2^768, canonical [0, p).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mnt753_params as P  # noqa: E402

NL, LB = 27, 28
RP_BITS = NL * LB          # 756
R_BITS = 768


def limbs(x, n, bits):
    m = (1 << bits) - 1
    out = []
    for _ in range(n):
        out.append(x & m)
        x >>= bits
    assert x == 0
    return out


def arr(vals, width=8):
    return "{" + ", ".join("0x%0*xu" % (width, v) for v in vals) + "}"


def arr64(vals):
    return "{" + ", ".join("0x%016xull" % v for v in vals) + "}"


def fp_const(p):
    rp = 1 << RP_BITS
    r = 1 << R_BITS
    inv28 = (-pow(p, -1, 1 << LB)) % (1 << LB)
    inv64 = (-pow(p, -1, 1 << 64)) % (1 << 64)
    d = {
        "p": limbs(p, NL, LB),
        "p2": limbs(2 * p, NL, LB),
        "one": limbs(rp % p, NL, LB),                       # 1 in internal form
        "k_in": limbs(pow(2, 2 * RP_BITS - R_BITS, p), NL, LB),   # file -> internal : 2^744
        "k_out": limbs(r % p, NL, LB),                      # internal -> file : 2^768
        "k_std": limbs(pow(pow(2, R_BITS - RP_BITS, p), -1, p), NL, LB),  # file Montgomery -> integer : 2^-12
        "r2p": limbs(rp * rp % p, NL, LB),                  # integer -> internal : R'^2
        "pm2": limbs(p - 2, NL, LB),                        # Fermat inversion exponent
        "inv": inv28,
        "p64": limbs(p, 12, 64),
        "inv64": inv64,
        "one64": limbs(r % p, 12, 64),                      # 1 in file form
        "r2_64": limbs(r * r % p, 12, 64),                  # R^2 mod p (file form of R)
        "r3_64": limbs(r * r * r % p, 12, 64),
    }
    return d


def emit_fp(name, d):
    s = "  { /* %s */\n" % name
    for k in ("p", "p2", "one", "k_in", "k_out", "k_std", "r2p", "pm2"):
        s += "    %s,\n" % arr(d[k], 7)
    s += "    0x%07xu,\n" % d["inv"]
    for k in ("p64",):
        s += "    %s,\n" % arr64(d[k])
    s += "    0x%016xull,\n" % d["inv64"]
    for k in ("one64", "r2_64", "r3_64"):
        s += "    %s,\n" % arr64(d[k])
    s += "  }"
    return s


def mont_file(x, p):
    return limbs(x * (1 << R_BITS) % p, 12, 64)


def pairing_constants(curve):
    """The constants of the ate pairing of one curve, all from the two moduli: with q the base-field modulus, r the group order and
    k the embedding degree, the loop count |q - r| and its sign (q < r), w0 = Phi_k(q) / r - q (w1 = 1), and the Frobenius constants
    gamma_i^j, gamma_i = NR^((q^i - 1) / k): Fq^k = Fq[w] / (w^k - NR), and the q^i-th power of sum a_j w^j is sum a_j gamma_i^j w^j."""
    q, r = (P.MOD_B, P.MOD_A) if curve == 0 else (P.MOD_A, P.MOD_B)
    k, nr = (4, P.MNT4_FQ2_NON_RESIDUE) if curve == 0 else (6, P.MNT6_FQ3_NON_RESIDUE)
    phi = q * q + 1 if k == 4 else q * q - q + 1
    assert phi % r == 0
    loop, w0 = abs(q - r), phi // r - q
    assert w0 == (-(loop - 1) if curve == 0 else loop)
    gamma = [pow(nr, (q ** i - 1) // k, q) for i in range(k)]
    assert all(pow(g, k, q) == 1 for g in gamma)
    psi_x, psi_y = subgroup_constants(curve, q, r, k, gamma[1])
    return {"q": q, "k": k, "loop": loop, "loop_neg": q < r, "w0_abs": abs(w0), "w0_neg": w0 < 0, "nr_inv": pow(nr, -1, q),
            "frob": [[pow(g, j, q) for j in range(k)] for g in gamma], "psi_x": psi_x, "psi_y": psi_y}


def subgroup_constants(curve, q, r, k, gamma1):
    """gamma_1^-2 and gamma_1^-3: the constants of psi = twist^-1 o Frobenius_q o twist on the twisted curve E'(F), F = Fq2 / Fq3,
    psi(x, y) = (x^q gamma_1^-2, y^q gamma_1^-3).  With w^2 = u = twist the untwisting map is (x, y) -> (x / w^2, y / w^3), so the
    constants are w^(2 (1 - q)) = twist^(1 - q) and w^(3 (1 - q)) = twist^(3 (1 - q) / 2); both lie in Fq.  psi satisfies
    X^2 - t X + q with t = q + 1 - r, and G2 is its eigenspace of the eigenvalue q = t - 1 (mod r): on G2::one() psi is the
    multiplication by q - r = t - 1, the (signed) ate loop count.  That fixes the sign of the y constant; all three are asserted."""
    import pyref
    C = pyref.Curve(curve)
    deg = k // 2
    psi_x, psi_y = pow(gamma1, -2, q), pow(gamma1, -3, q)
    twist = tuple(1 if j == 1 else 0 for j in range(deg))

    def f_pow(x, e):
        acc = C.f_one(x)
        for bit in bin(e)[2:]:
            acc = C.f_mul(acc, acc)
            if bit == "1":
                acc = C.f_mul(acc, x)
        return acc
    twist_inv = C.f_inv(twist)
    embed = lambda c: (c,) + (0,) * (deg - 1)
    assert f_pow(twist_inv, q - 1) == embed(psi_x)                 # twist^(1 - q), zero higher components
    assert f_pow(twist_inv, 3 * (q - 1) // 2) == embed(psi_y)      # twist^(3 (1 - q) / 2)
    # x^q in F: component c times gamma_1^(2 c) (the existing frob[1][2 c])
    frob = lambda x: tuple(x[c] * pow(gamma1, 2 * c, q) % q for c in range(deg))
    gx, gy = C.gen(2)
    psi_g = (tuple(v * psi_x % q for v in frob(gx)), tuple(v * psi_y % q for v in frob(gy)))
    want = C.mul(abs(q - r), (gx, gy), 2)
    if q < r:
        want = C.neg(want)
    assert C.on_curve(psi_g, 2) and psi_g == want                   # psi(G2::one()) == [q - r] G2::one()
    return psi_x, psi_y


def emit_pairing():
    rp = 1 << RP_BITS
    out = []
    out.append("// GENERATED by tools/gen_constants.py -- do not edit.  Every number follows from the two moduli of tools/mnt753_params.py:")
    out.append("// the ate loop count |q - r| and its sign (q < r), w0 = Phi_k(q) / r - q (w1 = 1), 1 / NR, and the Frobenius constants")
    out.append("// gamma_i^j with gamma_i = NR^((q^i - 1) / k) of Fq^k = Fq[w] / (w^k - NR), k = 4 (MNT4753, NR = 13) or 6 (MNT6753, NR = 11).")
    out.append("#pragma once")
    out.append("#include <stdint.h>")
    out.append('#include "mnt753_constants.h"')
    out.append("namespace mnt753 {")
    out.append("struct PairingConst {")
    out.append("  uint32_t loop_count[12];   // |q - r|, 32-bit words, little endian")
    out.append("  int loop_bits, loop_neg;   // its bit length; 1 if q < r (ate_is_loop_count_neg)")
    out.append("  uint32_t w0_abs[12];       // |w0| of the last chunk of the final exponent")
    out.append("  int w0_bits, w0_neg;")
    out.append("  uint32_t nr_inv[NL];       // 1 / NR, device form: the twist's inverse is u^(deg - 1) / NR")
    out.append("  uint32_t frob[6][6][NL];   // frob[i][j] = gamma_i^j, device form; entries with i or j >= k are zero")
    out.append("  uint32_t psi_x[NL], psi_y[NL];   // gamma_1^-2, gamma_1^-3, device form: psi(x, y) = (x^q psi_x, y^q psi_y) on the twist (subgroup test)")
    out.append("};")
    out.append("static constexpr PairingConst PAIRC[2] = {")
    for curve in (0, 1):
        c = pairing_constants(curve)
        q, k = c["q"], c["k"]
        dev = lambda x: arr(limbs(x * rp % q, NL, LB), 7)
        s = "  { /* %s */\n" % ("MNT4753" if curve == 0 else "MNT6753")
        s += "    %s,\n    %d, %d,\n" % (arr(limbs(c["loop"], 12, 32)), c["loop"].bit_length(), int(c["loop_neg"]))
        s += "    %s,\n    %d, %d,\n" % (arr(limbs(c["w0_abs"], 12, 32)), c["w0_abs"].bit_length(), int(c["w0_neg"]))
        s += "    %s,\n    {\n" % dev(c["nr_inv"])
        for i in range(6):
            row = [dev(c["frob"][i][j]) if i < k and j < k else arr([0] * NL, 7) for j in range(6)]
            s += "     {" + ",\n      ".join(row) + "}" + (",\n" if i < 5 else "\n")
        s += "    },\n    %s,\n    %s\n  }" % (dev(c["psi_x"]), dev(c["psi_y"])) + ("," if curve == 0 else "")
        out.append(s)
    out.append("};")
    out.append("}  // namespace mnt753")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "snark-challenge-prover-reference_amd", "csrc", "mnt753_pairing_constants.h")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", os.path.normpath(path))


def sqrt_constants(q, deg, nr):
    """Tonelli-Shanks constants of F = Fq[u] / (u^deg - nr) (deg 1: Fq itself): q^deg - 1 = 2^s t with t odd, the exponent (t - 1) / 2,
    and z^t for the first non-square z of a fixed walk (small integers, then u, u + 1, ...).  All asserted: z^((q^deg - 1) / 2) = -1,
    z^t has order exactly 2^s."""
    def mul(x, y):
        out = [0] * (2 * deg - 1)
        for i in range(deg):
            for j in range(deg):
                out[i + j] += x[i] * y[j]
        for k in range(2 * deg - 2, deg - 1, -1):
            out[k - deg] += nr * out[k]
        return tuple(v % q for v in out[:deg])

    def fpow(x, e):
        acc = (1,) + (0,) * (deg - 1)
        for bit in bin(e)[2:]:
            acc = mul(acc, acc)
            if bit == "1":
                acc = mul(acc, x)
        return acc
    order = q ** deg - 1
    s = (order & -order).bit_length() - 1
    t = order >> s
    one, minus_one = (1,) + (0,) * (deg - 1), (q - 1,) + (0,) * (deg - 1)
    walk = [(v,) + (0,) * (deg - 1) for v in range(2, 40)]
    if deg > 1:
        walk = [(v, 1) + (0,) * (deg - 2) for v in range(0, 40)] + walk
    z = next(c for c in walk if fpow(c, order // 2) == minus_one)
    zt = fpow(z, t)
    assert fpow(zt, 1 << (s - 1)) == minus_one and fpow(zt, 1 << s) == one
    return {"s": s, "e": (t - 1) // 2, "z": z, "zt": zt}


SQRT_WORDS = 70   # 32-bit words of the longest exponent: (t - 1) / 2 of Fq3 has 2229 bits


def emit_sqrt():
    """csrc/mnt753_sqrt_constants.h: the square-root constants of the four coordinate fields (csrc/fp_sqrt.hip.h)."""
    A, B = P.MOD_A, P.MOD_B
    rp = 1 << RP_BITS
    fields = (("Fq of MNT4753", B, 1, 0), ("Fq of MNT6753", A, 1, 0),
              ("Fq2 of MNT4753", B, 2, P.MNT4_FQ2_NON_RESIDUE), ("Fq3 of MNT6753", A, 3, P.MNT6_FQ3_NON_RESIDUE))
    out = []
    out.append("// GENERATED by tools/gen_constants.py -- do not edit.  Tonelli-Shanks constants of the four coordinate fields, from the two moduli")
    out.append("// of tools/mnt753_params.py: with |F| - 1 = 2^s t, t odd, the exponent (t - 1) / 2 and z^t for a non-square z (csrc/fp_sqrt.hip.h).")
    out.append("#pragma once")
    out.append("#include <stdint.h>")
    out.append('#include "mnt753_constants.h"')
    out.append("namespace mnt753 {")
    out.append("struct SqrtConst {")
    out.append("  int s;                     // 2-adicity of |F| - 1")
    out.append("  int e_bits;                // bit length of (t - 1) / 2")
    out.append("  uint32_t e[%d];            // (t - 1) / 2, 32-bit words, little endian" % SQRT_WORDS)
    out.append("  uint32_t zt[3][NL];        // z^t per component, device form; unused components zero")
    out.append("};")
    out.append("// index: 0 Fq of MNT4753, 1 Fq of MNT6753, 2 Fq2 of MNT4753, 3 Fq3 of MNT6753")
    out.append("static constexpr SqrtConst SQRTC[4] = {")
    for k, (name, q, deg, nr) in enumerate(fields):
        c = sqrt_constants(q, deg, nr)
        zt = list(c["zt"]) + [0] * (3 - deg)
        s = "  { /* %s: z = %s */\n" % (name, "(" + ", ".join(str(v) for v in c["z"]) + ")")
        s += "    %d, %d,\n    %s,\n    {" % (c["s"], c["e"].bit_length(), arr(limbs(c["e"], SQRT_WORDS, 32)))
        s += ",\n     ".join(arr(limbs(v * rp % q, NL, LB), 7) for v in zt) + "}\n  }" + ("," if k < 3 else "")
        out.append(s)
    out.append("};")
    out.append("}  // namespace mnt753")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "snark-challenge-prover-reference_amd", "csrc", "mnt753_sqrt_constants.h")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", os.path.normpath(path))


def main():
    A, B = P.MOD_A, P.MOD_B
    dA, dB = fp_const(A), fp_const(B)
    out = []
    out.append("// GENERATED by tools/gen_constants.py -- do not edit.  Source numbers: tools/mnt753_params.py")
    out.append("// (decimal literals of the reference's mnt4753_init.cpp / mnt6753_init.cpp, cited there).")
    out.append("#pragma once")
    out.append("#include <stdint.h>")
    out.append("namespace mnt753 {")
    out.append("constexpr int NL = %d;        // limbs of the device representation" % NL)
    out.append("constexpr int LB = %d;        // bits per device limb" % LB)
    out.append("constexpr uint32_t LMASK = 0x%xu;" % ((1 << LB) - 1))
    out.append("constexpr int MOD_A = 0;      // Fr of MNT4753, Fq of MNT6753")
    out.append("constexpr int MOD_B = 1;      // Fq of MNT4753, Fr of MNT6753")
    out.append("struct FpConst {")
    out.append("  uint32_t p[NL], p2[NL], one[NL], k_in[NL], k_out[NL], k_std[NL], r2p[NL], pm2[NL];")
    out.append("  uint32_t inv;             // -p^-1 mod 2^28")
    out.append("  uint64_t p64[12];         // modulus, 64-bit limbs (host / wire form)")
    out.append("  uint64_t inv64;           // -p^-1 mod 2^64")
    out.append("  uint64_t one64[12], r2_64[12], r3_64[12];")
    out.append("};")
    out.append("static constexpr FpConst FPC[2] = {")
    out.append(emit_fp("modulus A", dA) + ",")
    out.append(emit_fp("modulus B", dB))
    out.append("};")
    # FFT-related constants in file (R=2^768 Montgomery, 64-bit limb) form
    out.append("// Fr roots of unity and generators, file form (Montgomery R=2^768, 12x64-bit limbs).")
    out.append("struct FrDomainConst { int two_adicity; uint64_t root_of_unity[12]; uint64_t mult_gen[12]; };")
    g = P.MULTIPLICATIVE_GENERATOR
    # MNT6753 Fr: libff takes full_root_of_unity^(5^2) then squares down (field_utils.tcc:59-70); for a
    # power-of-two domain this equals a primitive 2^15-th root: full_root^25.
    rootB = pow(P.B_FULL_ROOT_OF_UNITY, P.B_SMALL_SUBGROUP_BASE ** P.B_SMALL_SUBGROUP_POWER, B)
    assert pow(rootB, 1 << 15, B) == 1 and pow(rootB, 1 << 14, B) != 1
    out.append("static constexpr FrDomainConst FRD[2] = {")
    out.append("  { %d, %s, %s }," % (P.A_TWO_ADICITY, arr64(mont_file(P.A_ROOT_OF_UNITY, A)), arr64(mont_file(g, A))))
    out.append("  { %d, %s, %s }" % (P.B_TWO_ADICITY, arr64(mont_file(rootB, B)), arr64(mont_file(g, B))))
    out.append("};")
    # the root the mixed-radix domains of MNT6753 start from: order 2^15 5^2 (mnt6753_init.cpp:76); FRD[1].root_of_unity is its 25th power
    full = P.B_FULL_ROOT_OF_UNITY
    order = (1 << P.B_TWO_ADICITY) * P.B_SMALL_SUBGROUP_BASE ** P.B_SMALL_SUBGROUP_POWER
    assert pow(full, order, B) == 1 and pow(full, order // 2, B) != 1 and pow(full, order // 5, B) != 1
    out.append("// mnt6753_Fr::full_root_of_unity, order 2^%d %d^%d, file form; small-subgroup base and power" % (P.B_TWO_ADICITY, P.B_SMALL_SUBGROUP_BASE, P.B_SMALL_SUBGROUP_POWER))
    out.append("static constexpr uint64_t FR_FULL_ROOT_B[12] = %s;" % arr64(mont_file(full, B)))
    out.append("constexpr int FR_SMALL_SUBGROUP_BASE_B = %d, FR_SMALL_SUBGROUP_POWER_B = %d;" % (P.B_SMALL_SUBGROUP_BASE, P.B_SMALL_SUBGROUP_POWER))
    # curve ids
    out.append("constexpr int CURVE_MNT4753 = 0;  // Fq = B, Fr = A, G2 over Fq2 (u^2 = 13)")
    out.append("constexpr int CURVE_MNT6753 = 1;  // Fq = A, Fr = B, G2 over Fq3 (u^3 = 11)")
    # the coefficient b of y^2 = x^3 + a x + b and b' of the twist, device form (b R' mod q, 28-bit limbs): the point check of
    # csrc/mnt753_validate.hip.  mnt4753_init.cpp:120,123 (b' = (0, b nr)), mnt6753_init.cpp:131,136 (b' = (b nr, 0, 0))
    rp = 1 << RP_BITS
    dev = lambda x, q: arr(limbs(x * rp % q, NL, LB), 7)
    b4n, b6n = P.MNT4_G1_B * P.MNT4_FQ2_NON_RESIDUE % B, P.MNT6_G1_B * P.MNT6_FQ3_NON_RESIDUE % A
    out.append("// curve coefficient b (G1) and twist coefficient b' (G2, per component; unused components zero), device form, by curve id")
    out.append("struct CurveBConst { uint32_t g1[NL]; uint32_t g2[3][NL]; };")
    out.append("static constexpr CurveBConst CURVE_B[2] = {")
    out.append("  { %s,\n    {%s,\n     %s,\n     %s} }," % (dev(P.MNT4_G1_B, B), dev(0, B), dev(b4n, B), dev(0, B)))
    out.append("  { %s,\n    {%s,\n     %s,\n     %s} }" % (dev(P.MNT6_G1_B, A), dev(b6n, A), dev(0, A), dev(0, A)))
    out.append("};")
    out.append("}  // namespace mnt753")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "snark-challenge-prover-reference_amd", "csrc", "mnt753_constants.h")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", os.path.normpath(path))
    # ---- oracle constants (plain C, 64-bit limbs) ----
    o = []
    o.append("/* GENERATED by tools/gen_constants.py -- do not edit.  Numbers from tools/mnt753_params.py, which cites the")
    o.append(" * reference's mnt4753_init.cpp / mnt6753_init.cpp line by line.  Index 0 = modulus A, 1 = modulus B. */")
    o.append("#pragma once")
    o.append("#include <stdint.h>")
    def c64(vals):
        return "{" + ", ".join("0x%016xULL" % v for v in vals) + "}"
    o.append("static const uint64_t ORACLE_MOD[2][12] = {%s,\n  %s};" % (c64(dA["p64"]), c64(dB["p64"])))
    o.append("static const uint64_t ORACLE_INV[2] = {0x%016xULL, 0x%016xULL};  /* -p^-1 mod 2^64 (mnt4753_init.cpp:54,81) */" % (dA["inv64"], dB["inv64"]))
    o.append("static const uint64_t ORACLE_ONE[2][12] = {%s,\n  %s};  /* R mod p */" % (c64(dA["one64"]), c64(dB["one64"])))
    o.append("static const uint64_t ORACLE_R2[2][12] = {%s,\n  %s};  /* Rsquared (mnt4753_init.cpp:52,79) */" % (c64(dA["r2_64"]), c64(dB["r2_64"])))
    o.append("static const uint64_t ORACLE_R3[2][12] = {%s,\n  %s};  /* Rcubed (mnt4753_init.cpp:53,80) */" % (c64(dA["r3_64"]), c64(dB["r3_64"])))
    o.append("static const int ORACLE_FR_S[2] = {%d, %d};  /* two-adicity of Fr: mnt4753_init.cpp:65, mnt6753_init.cpp:66 */" % (P.A_TWO_ADICITY, P.B_TWO_ADICITY))
    o.append("static const uint64_t ORACLE_FR_ROOT_A[12] = %s;  /* mnt4753_Fr::root_of_unity (mnt4753_init.cpp:69), Montgomery form */" % c64(mont_file(P.A_ROOT_OF_UNITY, A)))
    o.append("static const uint64_t ORACLE_FR_FULL_ROOT_B[12] = %s;  /* mnt6753_Fr::full_root_of_unity (mnt6753_init.cpp:76), Montgomery form */" % c64(mont_file(P.B_FULL_ROOT_OF_UNITY, B)))
    opath = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "mnt753_oracle_constants.h")
    with open(opath, "w") as f:
        f.write("\n".join(o) + "\n")
    print("wrote", os.path.normpath(opath))
    emit_pairing()
    emit_sqrt()


if __name__ == "__main__":
    main()

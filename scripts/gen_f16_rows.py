#!/usr/bin/env python3
"""Generate csrc/swbank_f16_rows.inc: asm text for one 8-row block of the f16 tile-kernel
column, for both gap models and both substitution lookups.

Merged gap matrix (the ScoreBank PE), scores as f16 multiples of 2^-11 so that the packed
add's [0, 1] clamp is max(0, x); per row, with M = max(0, H(i-1,j-1) + s) already computed:

    s'  = v_perm(...)                 substitution word of the next row (VOP3; LUT/profile)
    MO  = M + (-o)
    T   = X(prev row) + (-e)   -> Tl  T of the previous row (= G - e: what the right and lower
                                      cells read), written one group late
    M'  = clamp(Hl(old) + s')         next row's M
    H   = max(M, Tup, Tl)      -> Hl  (= max(M, I), I = max(Tup, Tl))
    X   = max(MO, Tup, Tl)            G = max(M - o, I)
    best = max(best, H(prev row), H)  every second row

Gotoh (ssearch36), E and F one step ahead and floored at 0:

    s'  = v_perm(...)
    D'  = Hl(old) + s'
    H   = max(D, El, F)      -> Hl
    EN  = El + (-e)
    HN  = H + (-o-e)
    FN  = F + (-e)
    El  = max(0, HN, EN)
    F   = max(0, HN, FN)              (F of the next row)
    best = max(best, H(prev row), H)  every second row

Lookups: LUT (DNA) `v_perm_b32 s, nv, lut[row], sel` with the row's LUT word in an SGPR;
profile (any alphabet, 2-byte f16 entries) `v_perm_b32 s, hi[w], lo[w], selk` with the two
target letters' profile words in VGPRs and a per-parity selector in an SGPR.

Mode "F" (profile, 4-byte words {s, 1.0} per letter and row): no lookup instruction at all.
The next row's diagonal add is one packed FMA that takes target A's entry from the low half of
A's word and target B's from the low half of B's word, the 1.0 in the other word's high half
being the multiplier:
    v_pk_fma_f16 D, a, b, h op_sel:[0,1,0] op_sel_hi:[1,0,1]
    D.lo = a.lo * b.hi + h.lo = sA + h.lo      D.hi = a.hi * b.lo + h.hi = sB + h.hi
(exact: every operand is an f16 multiple of 2^-11 in [-1, 1], one rounding; the clamp modifier
is max(0, x) as for the add; scripts/ubench/fma_opsel.hip checks both and the issue rate, which
equals v_pk_add_f16's).  So a profile row costs 7.5 VALU (Gotoh) / 5.5 (merged) per 2 cells like
the DNA letter-pair table, without a table per letter pair.

Skewed merged pair rows (SWK_F16SKEW_F/M/L, skew_pair_block below): cells in anti-diagonal
frames that restart every 8 rows, 4.75 VALU per row with the letter-pair table holding s + 2e
(s + 2e - 8e in a block's first row); SWK_F16SKEW8_F/L: the same rows with the running best in
eight accumulators named by frame mod 8, one move per column, 4.66 per row.

No two dependent packed (VOP3P) ops are adjacent (gfx950 needs a wait state between them;
v_perm_b32 -> VOP3P needs none), so a block needs no s_nop inside; LLVM adds one wait state
per asm block.  D alternates between Da/Db by row parity.  The last block of a column ends
with a row that has no successor: `s_nop 0` stands in for its next-row add.
usage: python scripts/gen_f16_rows.py   (rewrites the .inc)
"""
import os

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "smith-waterman-fpga-module_amd", "csrc", "swbank_f16_rows.inc")


def perm(mode, i):
    """substitution word of block row i+1 into S1"""
    if mode == "L":
        return f"v_perm_b32 %[S1], %[nv], %[tb{i}], %[sel]"
    w = (i + 1) // 2
    k = "%[selB]" if (i + 1) % 2 else "%[selA]"
    return f"v_perm_b32 %[S1], %[hi{w}], %[lo{w}], {k}"


FMA_SEL = "op_sel:[0,1,0] op_sel_hi:[1,0,1]"


def next_d(mode, i, dnext, clamp):
    """the diagonal add of block row i + 1 (into dnext) for mode F / pair / L,P (S1)"""
    c = " clamp" if clamp else ""
    if mode == "F":
        return [f"v_pk_fma_f16 {dnext}, %[fa{i}], %[fb{i}], %[h{i}] {FMA_SEL}{c}"]
    if mode == "pair":
        return [f"v_pk_add_f16 {dnext}, %[h{i}], %[p{i}]{c}"]
    return [perm(mode, i), f"v_pk_add_f16 {dnext}, %[h{i}], %[S1]{c}"]


def merged_block(mode, zdown, last, nrows=8):
    """Merged gap matrix with the clamp modifier: values are f16 multiples of 2^-11, so the
    [0, 1] clamp of v_pk_add_f16 is max(0, x) on everything the exact path reaches, and the
    diagonal add yields M = max(0, H(i-1,j-1) + s) directly.  Then I = max(Tup, Tl) never has
    to be formed on its own: H = max(M, Tup, Tl) and G = max(M - o, Tup, Tl) are one max3 each
    and T = G - e.  5.5 VALU per 2 cells (+ the substitution lookup).  T of row i is written
    one group late (after the next row's M - o), so no two dependent packed ops are adjacent.
    mode "L"/"P": perm lookups into S1; "pair": ready-made words p{i} (no lookup)."""
    out = []
    for i in range(nrows):
        dcur, dnext = ("%[Da]", "%[Db]") if i % 2 == 0 else ("%[Db]", "%[Da]")
        up = "%[up]" if i == 0 else ("%[noe]" if zdown else f"%[t{i - 1}]")
        final = last and i == nrows - 1
        if final:
            nxt = ["s_nop 0"]
        else:
            nd = next_d(mode, i, dnext, True)
            out += nd[:-1]  # (the perm of the L / P lookups)
            nxt = nd[-1:]
        if i == 0:
            out += nxt
            out.append(f"v_pk_add_f16 %[DN], {dcur}, %[no]")
        else:
            out.append(f"v_pk_add_f16 %[DN], {dcur}, %[no]")
            out.append(f"v_pk_add_f16 %[t{i - 1}], %[X], %[ne]")
            out += nxt
        out.append(f"v_pk_maximum3_f16 %[h{i}], {dcur}, {up}, %[t{i}]")
        out.append(f"v_pk_maximum3_f16 %[X], %[DN], {up}, %[t{i}]")
        if i % 2 == 1:
            out.append(f"v_pk_maximum3_f16 %[best], %[best], %[h{i - 1}], %[h{i}]")
    if nrows % 2 == 1:
        out.append("s_nop 0")
    out.append(f"v_pk_add_f16 %[t{nrows - 1}], %[X], %[ne]")
    return out


def gotoh_block(mode, last, nrows=8):
    """mode "L"/"P": perm lookups into S1; "pair": ready-made words p{i} (no lookup)."""
    out = []
    for i in range(nrows):
        dcur, dnext = ("%[Da]", "%[Db]") if i % 2 == 0 else ("%[Db]", "%[Da]")
        final = last and i == nrows - 1
        if final:
            out.append("s_nop 0")
        else:
            out += next_d(mode, i, dnext, False)
        out.append(f"v_pk_maximum3_f16 %[h{i}], {dcur}, %[t{i}], %[F]")
        out.append(f"v_pk_add_f16 %[EN], %[t{i}], %[ne]")
        out.append(f"v_pk_add_f16 %[HN], %[h{i}], %[noe]")
        out.append("v_pk_add_f16 %[FN], %[F], %[ne]")
        out.append(f"v_pk_maximum3_f16 %[t{i}], 0, %[HN], %[EN]")
        out.append("v_pk_maximum3_f16 %[F], 0, %[HN], %[FN]")
        if i % 2 == 1:
            out.append(f"v_pk_maximum3_f16 %[best], %[best], %[h{i - 1}], %[h{i}]")
    return out


def pair_block(first, last, nrows=8):
    """Pair-profile block (DNA, merged gaps): the substitution words of both targets come
    ready-made from an LDS table of letter pairs, word p{i} = s(row i+1) for (lo, hi), so
    there is no v_perm per row: 5.5 VALU per 2 cells.  Da carries M of the block's first row
    in and of the next block's first row out; the first block computes it from dg + pw."""
    out = ["v_pk_add_f16 %[Da], %[dg], %[pw] clamp"] if first else []
    return out + merged_block("pair", False, last, nrows)

def pair_gotoh_block(first, last, nrows=8):
    """Pair-profile block, Gotoh (DNA): as gotoh_block with the substitution words p{i} from
    the letter-pair table, 7.5 VALU per 2 cells instead of 8.5.  F runs down the column in
    %[F]; the first block computes row 0's D from dg + pw (the clamp is harmless: H is the max
    of D and the floored E, F)."""
    out = ["v_pk_add_f16 %[Da], %[dg], %[pw] clamp"] if first else []
    return out + gotoh_block("pair", last, nrows)


SKEW_ACC = 8       # accumulators of the running best (csrc: SWK_SKEW_ACC)
SKEW_ACC_TRIM = 4  # ... of the trimmed kernel, which leaves a chunk at any column (SWK_SKEW_ACC_TRIM)


def _regs(ln):
    """(destination, sources) of one generated line."""
    op, rest = ln.split(None, 1)
    ops = [x.strip() for x in rest.split(",")]
    return ops[0], ops[1:]


def check_no_adjacent_dependence(lines):
    """No instruction reads the register the one before it wrote."""
    for a, b in zip(lines, lines[1:]):
        if a.startswith("s_nop") or b.startswith("s_nop"):
            continue
        assert _regs(a)[0] not in _regs(b)[1], (a, b)
    return lines


def skew_pair_block(kind, nacc=SKEW_ACC_TRIM, nrows=8):
    """Pair-profile block in block frames (DNA, merged gaps, DESIGN 3.1 "skewed rows"): cell
    (i, j) is held with the offset c_f = e (f - 1), f = (i mod 8) + j, so the gap extension is
    paid by the frame and a row is 4 VALU:

        A'  = Hl(old) + p            next row's A = H^(i-1,j-1) + (s + 2e)   (no clamp)
        T~  = max3(AO, Tup, Tl) -> Tl   (= G + c_f: what the right and lower cells read)
        AO' = A' + (-o)              next row's A - o
        H^  = max3(T~, A, c_f)  -> Hl   c_f: the frame's floor (H = 0), an SGPR per row

    A block's first row sits 7 frames before the row above it: its table word holds s + 2e - 8e
    (no instruction) and its Tup is shifted once, Tup + (-8e).  kind "F" (a column's first
    block) forms row 0's A and A - o from dg + pw and shifts the ring entry in place; every
    block but the last ends by shifting its last T~ into Db for the block below, which reads it
    before it writes Db ("M", "L": Da, AO and Db come in).  AO runs one row ahead.

    The best: rows u, u + 8, u + 16, u + 24 of a column share frame u + j, so two max3 fold the
    four (g: rows 0-7, k: 8-15, m: 16-23 of the column, h: the last block's own) into
    accumulator b[u / 2], which makes one + e move per column, between its classes 2a and
    2a + 1, and none to the next column (class 2a of column j + 1 has the frame of class 2a + 1
    of column j).  The folds go into the last block, between the rows' dependent pairs; the
    last accumulator's move and class 7 (row 7 of the last block ends the column) into the
    first block of the next column, before it overwrites row 7: x, y, z = rows 15, 23, 31.
    16 max3 and 4 adds per column: 4.75 VALU per row with the 4 shifts.

    nacc = 8 (SWK_F16SKEW8_F / _L; the middle blocks are the same): one accumulator per frame,
    named by the frame mod 8, so the accumulator of class u in column j is b[(u + j) mod 8] and
    stays with its frame from column to column.  Frame j leaves after column j and its
    accumulator takes frame j + 8, class 7 of column j + 1: one + 8e move per column (- 8e
    negated by the instruction's modifiers), run with class 7's delayed fold in the next first
    block.  The text is the same for every column: the caller binds the operands by class,
    %[b0] .. %[b6] = the accumulators of classes 0-6 of this column (b[(u + jj) mod 8]), %[bf]
    = the one of the previous column's class 7 (b[(jj + 6) mod 8]), %[bm] = the one that moves
    (b[(jj + 7) mod 8], the previous column's class 0); after the 8 columns of a chunk the
    names are back where they were.  16 max3 and 1 add per column."""
    assert nrows == 8 and nacc in (4, 8)
    rows = []  # per row: [nd, tt, ao, hh]
    for i in range(nrows):
        dcur, dnext = ("%[Da]", "%[Db]") if i % 2 == 0 else ("%[Db]", "%[Da]")
        up = ("%[up]" if kind == "F" else "%[Db]") if i == 0 else f"%[t{i - 1}]"
        rows.append([f"v_pk_add_f16 {dnext}, %[h{i}], %[p{i}]",
                     f"v_pk_maximum3_f16 %[t{i}], %[AO], {up}, %[t{i}]",
                     f"v_pk_add_f16 %[AO], {dnext}, %[no]",
                     f"v_pk_maximum3_f16 %[h{i}], %[t{i}], {dcur}, %[c{i}]"])
    shift = f"v_pk_add_f16 %[Db], %[t{nrows - 1}], %[ne8]"
    if kind == "F":
        bf = "%[b3]" if nacc == 4 else "%[bf]"
        move = ("v_pk_add_f16 %[b3], %[b3], %[e1]" if nacc == 4 else
                "v_pk_add_f16 %[bm], %[bm], %[ne8] neg_lo:[0,1] neg_hi:[0,1]")
        nd, tt, ao, hh = rows[0]
        out = ["v_pk_add_f16 %[Da], %[dg], %[pw]", "v_pk_add_f16 %[up], %[up], %[ne8]", nd,
               "v_pk_add_f16 %[AO], %[Da], %[no]", move, tt, ao,
               f"v_pk_maximum3_f16 {bf}, {bf}, %[h7], %[x]", hh]
        nd, tt, ao, hh = rows[1]
        out += [nd, tt, f"v_pk_maximum3_f16 {bf}, {bf}, %[y], %[z]", ao, hh]
        for r in rows[2:]:
            out += r
        return check_no_adjacent_dependence(out + [shift])
    nd, tt, ao, hh = rows[0]
    base = [tt, nd, hh, ao]  # (Db: the shifted Tup, read before the next row's A goes there)
    if kind == "M":
        for r in rows[1:]:
            base += r
        return check_no_adjacent_dependence(base + [shift])
    assert kind == "L"
    for r in rows[1:-1]:
        base += r
    base += [rows[-1][1], rows[-1][3]]  # the column's last row has no successor
    # the folds: per accumulator a chain; (line, the row of this block it waits for or None)
    chains = []
    for a in range(nacc if nacc == 4 else nrows - 1):
        u, v, b = (2 * a, 2 * a + 1, f"%[b{a}]") if nacc == 4 else (a, None, f"%[b{a}]")
        ch = [(f"v_pk_maximum3_f16 {b}, {b}, %[g{u}], %[k{u}]", None),
              (f"v_pk_maximum3_f16 {b}, {b}, %[m{u}], %[h{u}]", u)]
        if nacc == 4 and a < nacc - 1:
            ch += [(f"v_pk_add_f16 {b}, {b}, %[e1]", None),
                   (f"v_pk_maximum3_f16 {b}, {b}, %[g{v}], %[k{v}]", None),
                   (f"v_pk_maximum3_f16 {b}, {b}, %[m{v}], %[h{v}]", v)]
        chains.append(ch)
    nch = len(chains)
    out, done = [], set()  # done: rows of this block whose H^ is written
    turn = 0
    for ln in base:
        out.append(ln)
        d = _regs(ln)[0]
        if ln.startswith("v_pk_maximum3") and d.startswith("%[h"):
            done.add(int(d[3:-1]))
        for k in range(nch):  # one fold after each row instruction, accumulators in turn
            ch = chains[(turn + k) % nch]
            if not ch:
                continue
            f, wait = ch[0]
            if (wait is None or wait in done) and _regs(out[-1])[0] not in _regs(f)[1]:
                out.append(ch.pop(0)[0])
                turn = (turn + k + 1) % nch
                break
    assert not any(chains), chains
    return check_no_adjacent_dependence(out)


def fmt(lines):
    return "".join(f'  "{ln}\\n\\t" \\\n' for ln in lines) + '  ""\n'


def main():
    parts = ["// Generated by scripts/gen_f16_rows.py -- do not edit.\n"
             "// 8-row blocks of the f16 tile-kernel column (see the generator's docstring).\n"]
    for mode in ("L", "P"):
        for zd in (0, 1):
            for last in (0, 1):
                parts.append(f"#define SWK_F16M_{mode}_Z{zd}_L{last} \\\n" +
                             fmt(merged_block(mode, zd, last)))
        for last in (0, 1):
            parts.append(f"#define SWK_F16G_{mode}_L{last} \\\n" + fmt(gotoh_block(mode, last)))
    # whole-column blocks for the DNA LUT merged variants (R = 16, 32): one asm block
    # per column, so LLVM adds one wait state per column instead of one per 8 rows; the
    # operand lists are generated too (h/t/tb numbered 0..R-1)
    for R in (16, 32):
        parts.append(f"#define SWK_F16M_L_Z0_COL{R} \\\n" + fmt(merged_block("L", 0, 1, R)))
        hts = ", ".join([f'[h{i}] "+v"(Hl[{i}])' for i in range(R)] +
                        [f'[t{i}] "+v"(Xl[{i}])' for i in range(R)])
        parts.append(f"#define SWK_F16_COL{R}_HT {hts}\n")
        tbs = ", ".join(f'[tb{i}] "s"(lk.tab[{min(i + 1, R - 1)}])' for i in range(R))
        parts.append(f"#define SWK_F16_COL{R}_TB {tbs}\n")
    # pair-profile blocks: first (with the column prologue), middle, last (final row)
    parts.append("#define SWK_F16PAIR_F \\\n" + fmt(pair_block(True, False)))
    parts.append("#define SWK_F16PAIR_M \\\n" + fmt(pair_block(False, False)))
    parts.append("#define SWK_F16PAIR_L \\\n" + fmt(pair_block(False, True)))
    parts.append("#define SWK_F16PAIRG_F \\\n" + fmt(pair_gotoh_block(True, False)))
    parts.append("#define SWK_F16PAIRG_M \\\n" + fmt(pair_gotoh_block(False, False)))
    parts.append("#define SWK_F16PAIRG_L \\\n" + fmt(pair_gotoh_block(False, True)))
    for kind in "FML":
        parts.append(f"#define SWK_F16SKEW_{kind} \\\n" + fmt(skew_pair_block(kind)))
    for kind in "FL":  # (the middle blocks hold nothing of the best)
        parts.append(f"#define SWK_F16SKEW8_{kind} \\\n" +
                     fmt(skew_pair_block(kind, SKEW_ACC)))
    # mode F (profile words {s, 1.0}: one packed FMA per row, no lookup), 8-row blocks
    for last in (0, 1):
        parts.append(f"#define SWK_F16M_F_Z0_L{last} \\\n" + fmt(merged_block("F", 0, last)))
        parts.append(f"#define SWK_F16G_F_L{last} \\\n" + fmt(gotoh_block("F", last)))
    # 4- and 2-row single blocks (the wave kernel's K = 4, and K = 2 of its split tail: a
    # whole column in one block)
    for nr in (4, 2):
        for mode in ("L", "P"):
            parts.append(f"#define SWK_F16M_{mode}_Z0_L1_R{nr} \\\n" +
                         fmt(merged_block(mode, 0, 1, nr)))
            parts.append(f"#define SWK_F16G_{mode}_L1_R{nr} \\\n" + fmt(gotoh_block(mode, 1, nr)))
    open(OUT, "w").write("".join(parts))
    print("wrote", OUT)


if __name__ == "__main__":
    main()

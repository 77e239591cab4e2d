#!/usr/bin/env python3
"""Generate mini_nbody_amd/csrc/mutual_loop_gfx950.inc — the hand-scheduled unit loop of the mutual pairing (csrc/mutual.hip).

What it replaces: hipcc's schedule of the systolic step issued at 3.18 SIMD cycles per VALU instruction against the 2.73 of the ordered loop
(profiles/r18_mutual_pairing.md §A), because it controls none of the three hardware facts tools/gen_force_loop.py is built on:
  * an instruction whose three VGPR source reads have the same parity costs 4 cycles instead of 2: the temporaries are pinned, t/u even and
    dx/dy/dz odd, which settles every fma here whatever the parity of the accumulators;
  * v_rsq_f32 costs ~9.5 cycles when uniform 8-byte instructions start at 4 mod 8 bytes and ~24 at 0 mod 8: every instruction from the
    .p2align on is 8 bytes or one of a pair of 4-byte scalar instructions, and every 8-byte one starts at 4 mod 8;
  * a transcendental needs a wait state before its consumer: per row the order is
        sub sub sub | fmaak fma fma | rsq | 6 accumulating fma of the PREVIOUS row (3 direct, 3 mirrored) | mul mul
    and row 0, which has no previous row inside the step (the shifts stand between the steps), takes row 1's three subtractions instead.
    Priced against the other orders considered in profiles/r19_microbench_mutual_step.txt (tools/gen_streams.py, streams mstep_*).

One asm statement is a whole unit (row block A against `count` source blocks): the 96 row registers, the stream registers and the temporaries
never leave their physical registers, and hipcc allocates nothing around the loop.

  VGPRs  v8-v55 x, y, z of the lane's 16 rows | v56-v103 their direct sums | v104-v106 the source this lane holds | v107 256 * lane |
         v[108:111] its mirrored sums and a zero: the store tuple of lane 63 | v112-v123 temporaries | v[124:127] the flush's store tuple
  SGPRs  s[36:51], s[52:67] two buffers of four sources (s_load_dwordx16, alternating); the rest below (PTR ... SAVE)

  step   (the bookkeeping is wave-uniform, so it runs on the scalar unit: the step index of lane l is t - l)
         exec = all:   six v_mov_b32_dpp wave_shr:1 in place — lane 0 keeps its source (overwritten next), bound_ctrl gives its mirrored sums 0
         exec = lane 0: three v_mov_b32 of the new source from the SGPR buffer
         exec = MASK:  the 240 pair instructions.  MASK = (MASK << 1) | INBIT is the stream's occupancy of the array: it fills in the first
                       63 steps of a unit and drains in the last 64 (INBIT = 0), so fill and drain need no code of their own
         exec = MASK & lane 63 (0 in the diagonal unit): global_store_dwordx4 of the leaving mirrored sums at TM, TM += 16
  flush  lane l meets the end of a source block l steps after lane 0: BEFORE step j < 64 of every block but a unit's first, lane j stores its
         16 direct sums (T[previous block][its rows]) and zeroes them, exec = that one lane.  The code stands in every step behind a scalar
         compare-and-branch that 960 steps in 1024 take (option one of the two the design allowed: nothing is copied in or out of the loop).
         Lane 63's flush is also where TM moves on to the block that has reached lane 63.
  blocks count source blocks of 1024 steps, then a drain block of 64 steps that injects the first words of the source array (never used).
         The load after a block's last group reads that group again (STRIDE = 0), so nothing is read past a block.
The arithmetic and its order are run_unit's of the compiled form, i.e. pair_f32<0>'s per row, rows ascending in both accumulating chains.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "mini_nbody_amd", "csrc", "mutual_loop_gfx950.inc")

ROWS = 16
SOFT_BITS = 0x3089705F             # nbody_args.hpp kSoftBits
XI = [8 + r for r in range(ROWS)]
YI = [24 + r for r in range(ROWS)]
ZI = [40 + r for r in range(ROWS)]
AX = [56 + r for r in range(ROWS)]
AY = [72 + r for r in range(ROWS)]
AZ = [88 + r for r in range(ROWS)]
SX, SY, SZ = 104, 105, 106
LOFF = 107                         # 256 * lane: the lane's 16 rows as a byte offset
MQ = 108                           # v[108:111] = mx my mz 0
T = [112, 114]                     # d2 / inv / inv3 (even), alternating with the row
U = 116                            # inv^2 (even)
U2 = 118                           # the second chain's inv^2 in the interleaved candidate (microbenchmark only)
D = [(113, 115, 117), (119, 121, 123)]   # dx dy dz (odd), alternating with the row
FQ = 124                           # v[124:127] = ax ay az 0 of the row being flushed
LAND = 56                          # the prologue loads 8 rows at a time into v[56:87] (the accumulators, zeroed afterwards)
VGPR_LO, VGPR_HI = 8, 127

A_BASE, B_BASE = 36, 52
PTR, TM, FB, MASK, L63 = 34, 68, 70, 72, 74      # pairs
INBIT, FL, CNT, BI, BLK, NB, N16, STRIDE = 76, 77, 78, 79, 80, 81, 82, 83
SRC, TMB, TMN, TABA = 84, 86, 88, 90             # pairs
T0, T1, S128 = 92, 93, 94
SAVE = 96                                         # pair: exec on entry
GROUP = 8                                         # steps per iteration of the inner loop
HEAD = 60                                         # the inner loop's head, bytes past a 64-byte line

DPP = "v_mov_b32_dpp v%d, v%d wave_shr:1 row_mask:0xf bank_mask:0xf"


def sp(r):
    return "s[%d:%d]" % (r, r + 1)


def front(r, sx=SX, sy=SY, sz=SZ):
    """row r up to its v_rsq_f32: pair_f32<0>'s differences and d2 chain"""
    t, (dx, dy, dz) = T[r & 1], D[r & 1]
    return sub(r, sx, sy, sz) + [
        "v_fmaak_f32 v%d, v%d, v%d, 0x%08x" % (t, dz, dz, SOFT_BITS),
        "v_fma_f32 v%d, v%d, v%d, v%d" % (t, dy, dy, t),
        "v_fma_f32 v%d, v%d, v%d, v%d" % (t, dx, dx, t),
        "v_rsq_f32_e64 v%d, v%d" % (t, t)]


def sub(r, sx=SX, sy=SY, sz=SZ):
    dx, dy, dz = D[r & 1]
    return ["v_sub_f32_e64 v%d, v%d, v%d" % (dx, sx, XI[r]), "v_sub_f32_e64 v%d, v%d, v%d" % (dy, sy, YI[r]),
            "v_sub_f32_e64 v%d, v%d, v%d" % (dz, sz, ZI[r])]


def cube(r, u=U):
    t = T[r & 1]
    return ["v_mul_f32_e64 v%d, v%d, v%d" % (u, t, t), "v_mul_f32_e64 v%d, v%d, v%d" % (t, t, u)]


def acc(r):
    """the direct side fma(d, inv3, a_r), then the mirrored side fma(-d, inv3, m)"""
    t, (dx, dy, dz) = T[r & 1], D[r & 1]
    return ["v_fma_f32 v%d, v%d, v%d, v%d" % (AX[r], dx, t, AX[r]), "v_fma_f32 v%d, v%d, v%d, v%d" % (AY[r], dy, t, AY[r]),
            "v_fma_f32 v%d, v%d, v%d, v%d" % (AZ[r], dz, t, AZ[r]),
            "v_fma_f32 v%d, -v%d, v%d, v%d" % (MQ, dx, t, MQ), "v_fma_f32 v%d, -v%d, v%d, v%d" % (MQ + 1, dy, t, MQ + 1),
            "v_fma_f32 v%d, -v%d, v%d, v%d" % (MQ + 2, dz, t, MQ + 2)]


def pairs():
    """the 240 pair instructions of a step, one chain: the product order"""
    ins = front(0) + sub(1) + cube(0)
    ins += front(1)[3:] + acc(0) + cube(1)
    for r in range(2, ROWS):
        ins += front(r) + acc(r - 1) + cube(r)
    return ins + acc(ROWS - 1)


def shifts():
    return [DPP % (SX, SX), DPP % (SY, SY), DPP % (SZ, SZ)] + [(DPP + " bound_ctrl:1") % (MQ + k, MQ + k) for k in range(3)]


def inject(sbase, k):
    return ["v_mov_b32_e64 v%d, s%d" % (v, sbase + 4 * k + c) for c, v in enumerate((SX, SY, SZ))]


def flush():
    """lane FL stores its 16 direct sums to FB + 256 * lane and zeroes them; lane 63's flush moves TM on to the block that has reached it"""
    ins = ["s_lshl_b64 exec, 1, s%d" % FL, "s_cmp_eq_u32 s%d, 63" % FL,
           "s_cselect_b64 %s, %s, %s" % (sp(TM), sp(TMN), sp(TM)), "s_nop 0"]
    for r in range(ROWS):
        ins += ["v_mov_b32_e64 v%d, v%d" % (FQ, AX[r]), "v_mov_b32_e64 v%d, v%d" % (FQ + 1, AY[r]), "v_mov_b32_e64 v%d, v%d" % (FQ + 2, AZ[r]),
                "global_store_dwordx4 v%d, v[%d:%d], %s offset:%d" % (LOFF, FQ, FQ + 3, sp(FB), 16 * r),
                "v_mov_b32_e64 v%d, 0" % AX[r], "v_mov_b32_e64 v%d, 0" % AY[r], "v_mov_b32_e64 v%d, 0" % AZ[r]]
    return ins


def step(sbase, k):
    ins = ["s_cmp_lt_u32 s%d, 64" % FL, "s_cbranch_scc0 5f"] + flush() + ["5:"]
    ins += ["s_mov_b64 exec, -1", "s_add_u32 s%d, s%d, 1" % (FL, FL)] + shifts()
    ins += ["s_mov_b64 exec, 1", "s_lshl_b64 %s, %s, 1" % (sp(MASK), sp(MASK))] + inject(sbase, k)
    ins += ["s_or_b32 s%d, s%d, s%d" % (MASK, MASK, INBIT), "s_mov_b64 exec, %s" % sp(MASK)] + pairs()
    ins += ["s_and_b64 exec, %s, %s" % (sp(MASK), sp(L63)), "s_nop 0",
            "global_store_dwordx4 v%d, v[%d:%d], %s" % (MQ + 3, MQ, MQ + 3, sp(TM)),
            "s_add_u32 s%d, s%d, 16" % (TM, TM), "s_addc_u32 s%d, s%d, 0" % (TM + 1, TM + 1)]
    return ins


def prologue():
    ins = ["s_mov_b64 %s, exec" % sp(SAVE),
           "s_mov_b64 %s, %%[src]" % sp(SRC), "s_mov_b32 s%d, %%[first]" % BLK, "s_mov_b32 s%d, %%[count]" % BI, "s_mov_b32 s%d, %%[nb]" % NB,
           "s_lshl_b32 s%d, %%[n], 4" % N16,                                   # bytes of one table row: n <= 2^26
           "s_lshl_b32 s%d, %%[a], 14" % T0,                                   # row block A as a byte offset: A < 2^16
           "s_mov_b64 %s, %%[table]" % sp(TABA), "s_add_u32 s%d, s%d, s%d" % (TABA, TABA, T0), "s_addc_u32 s%d, s%d, 0" % (TABA + 1, TABA + 1),
           "s_mov_b64 %s, %%[table]" % sp(TMB), "s_mul_i32 s%d, %%[a], s%d" % (T1, N16), "s_mul_hi_u32 s%d, %%[a], s%d" % (S128, N16),
           "s_add_u32 s%d, s%d, s%d" % (TMB, TMB, T1), "s_addc_u32 s%d, s%d, s%d" % (TMB + 1, TMB + 1, S128),      # T[A]
           # lane 63 first holds a source at step 63: TM starts 63 words before the first block's first word (not stored to until then)
           "s_lshl_b32 s%d, s%d, 14" % (T1, BLK), "s_add_u32 s%d, s%d, s%d" % (TM, TMB, T1), "s_addc_u32 s%d, s%d, 0" % (TM + 1, TMB + 1),
           "s_sub_u32 s%d, s%d, 0x%x" % (TM, TM, 63 * 16), "s_subb_u32 s%d, s%d, 0" % (TM + 1, TM + 1),
           "s_mov_b64 %s, %s" % (sp(TMN), sp(TM)), "s_mov_b64 %s, %s" % (sp(FB), sp(TABA)),
           "s_mov_b64 %s, 0" % sp(MASK),
           "s_mov_b32 s%d, 0" % L63, "s_mov_b32 s%d, 0x80000000" % (L63 + 1), "s_cmp_eq_u32 %[d0], 0",
           "s_cselect_b32 s%d, 0, s%d" % (L63 + 1, L63 + 1),                   # the diagonal unit stores no mirrored sum
           "s_mov_b32 s%d, 1" % INBIT, "s_movk_i32 s%d, 0x40" % FL, "s_movk_i32 s%d, 0x80" % S128,
           "v_lshlrev_b32_e32 v%d, 8, %%[lane]" % LOFF,
           "s_add_u32 s%d, s%d, s%d" % (T0, SRC, T0), "s_addc_u32 s%d, s%d, 0" % (T1, SRC + 1)]                    # the lane's rows: src + A
    for half in range(2):
        for q in range(8):
            ins.append("global_load_dwordx4 v[%d:%d], v%d, %s offset:%d" % (LAND + 4 * q, LAND + 4 * q + 3, LOFF, sp(T0), 16 * (8 * half + q)))
        ins.append("s_waitcnt vmcnt(0)")
        for q in range(8):
            r = 8 * half + q
            ins += ["v_mov_b32_e32 v%d, v%d" % (dst, LAND + 4 * q + c) for c, dst in enumerate((XI[r], YI[r], ZI[r]))]
    ins += ["v_mov_b32_e32 v%d, 0" % v for v in AX + AY + AZ + [SX, SY, SZ, MQ, MQ + 1, MQ + 2, MQ + 3, FQ + 3]]
    return ins


def build():
    ins = prologue() + [".p2align 6"]
    # ---- one block of the stream: BI source blocks are left; 0 = the drain
    blk = ["2:",
           "s_waitcnt lgkmcnt(0)",                                             # the load the last group left in flight lands before the next is issued
           "s_cmp_eq_u32 s%d, 0" % BI, "s_cbranch_scc1 3f",
           "s_lshl_b32 s%d, s%d, 14" % (T0, BLK), "s_movk_i32 s%d, 0x%x" % (CNT, 1024 // GROUP),
           "s_add_u32 s%d, s%d, s%d" % (PTR, SRC, T0), "s_addc_u32 s%d, s%d, 0" % (PTR + 1, SRC + 1),
           "s_add_u32 s%d, s%d, s%d" % (TMN, TMB, T0), "s_addc_u32 s%d, s%d, 0" % (TMN + 1, TMB + 1),      # where TM goes when this block reaches lane 63
           "s_branch 4f",
           "3:",
           "s_mov_b64 %s, %s" % (sp(PTR), sp(SRC)), "s_mov_b32 s%d, 0" % INBIT, "s_movk_i32 s%d, 0x%x" % (CNT, 64 // GROUP),
           "4:",
           "s_load_dwordx16 s[%d:%d], %s, 0x0" % (A_BASE, A_BASE + 15, sp(PTR))]
    nbytes = sum(size(i) for i in blk)
    pad = ((HEAD - nbytes) % 64) // 4
    assert (nbytes + 4 * pad) % 64 == HEAD
    ins += ["s_nop 0"] * pad + blk
    ins += ["1:",
            "s_waitcnt lgkmcnt(0)", "s_sub_u32 s%d, s%d, 1" % (CNT, CNT),
            "s_cmp_eq_u32 s%d, 0" % CNT, "s_cselect_b32 s%d, 0, s%d" % (STRIDE, S128),     # the last group's successor: itself
            "s_load_dwordx16 s[%d:%d], %s, 0x40" % (B_BASE, B_BASE + 15, sp(PTR))]
    for k in range(4):
        ins += step(A_BASE, k)
    ins += ["s_add_u32 s%d, s%d, s%d" % (PTR, PTR, STRIDE), "s_addc_u32 s%d, s%d, 0" % (PTR + 1, PTR + 1),
            "s_waitcnt lgkmcnt(0)", "s_nop 0",
            "s_load_dwordx16 s[%d:%d], %s, 0x0" % (A_BASE, A_BASE + 15, sp(PTR))]
    for k in range(4):
        ins += step(B_BASE, k)
    ins += ["s_cmp_lg_u32 s%d, 0" % CNT, "s_cbranch_scc1 1b"]
    # ---- the block is through lane 0: after the drain the unit is done; else the next block's first 64 steps flush this one
    ins += ["s_cmp_eq_u32 s%d, 0" % BI, "s_cbranch_scc1 6f",
            "s_sub_u32 s%d, s%d, 1" % (BI, BI), "s_mov_b32 s%d, 0" % FL,
            "s_mul_i32 s%d, s%d, s%d" % (T0, BLK, N16), "s_mul_hi_u32 s%d, s%d, s%d" % (T1, BLK, N16),
            "s_add_u32 s%d, s%d, s%d" % (FB, TABA, T0), "s_addc_u32 s%d, s%d, s%d" % (FB + 1, TABA + 1, T1),            # T[this block][rows of A]
            "s_add_u32 s%d, s%d, 1" % (BLK, BLK), "s_cmp_ge_u32 s%d, s%d" % (BLK, NB),
            "s_cselect_b32 s%d, s%d, 0" % (T0, NB), "s_sub_u32 s%d, s%d, s%d" % (BLK, BLK, T0),                          # the blocks wrap past nb
            "s_branch 2b", "s_nop 0",
            "6:",
            "s_waitcnt vmcnt(0) lgkmcnt(0)", "s_mov_b64 exec, %s" % sp(SAVE)]
    return ins


def size(i):
    """bytes of an instruction as written here: scalar instructions carry no 32-bit literal, VALU ones are VOP3, VOP2 + literal or DPP"""
    if i.endswith(":"):
        return 0
    op = i.split()[0]
    if op.startswith("s_load") or op.startswith("global_"):
        return 8
    if op.startswith("s_"):
        for x in re.split(r"[ ,]+", i)[1:]:      # no 32-bit literal: registers, labels and inline constants only
            assert re.fullmatch(r"s\d+|s\[\d+:\d+\]|exec|\d[fb]|-?\d+|0x[0-9a-f]+|vmcnt\(0\)|lgkmcnt\(0\)", x), i
            if re.fullmatch(r"-?\d+", x):
                assert -16 <= int(x) <= 64, i
            if x.startswith("0x"):
                assert op in ("s_movk_i32",), i
        return 4
    assert op.startswith("v_")
    assert op.endswith("_e64") or op in ("v_fma_f32", "v_fmaak_f32", "v_mov_b32_dpp"), i
    return 8


def vsrc(i):
    """VGPRs an instruction reads (a DPP move reads its destination as `old`)"""
    regs = [int(x) for x in re.findall(r"\bv(\d+)\b", i)]
    m = re.search(r"v\[(\d+):(\d+)\]", i)
    if m:
        regs += list(range(int(m.group(1)), int(m.group(2)) + 1))
    op = i.split()[0]
    if op.startswith("global_store"):
        return regs
    return regs if op == "v_mov_b32_dpp" else regs[1:]


def vdst(i):
    op = i.split()[0]
    if not op.startswith("v_"):
        return []
    return [int(re.search(r"\bv(\d+)\b", i).group(1))]


def check(ins):
    """the rules the stream is built on, from the .p2align on"""
    body = [i for i in ins[ins.index(".p2align 6") + 1:]]
    at = 0
    head = None
    for i in body:
        if i == "1:":
            head = at % 64
        n = size(i)
        if n == 8:
            assert at % 8 == 4, (at, i)                 # every 8-byte instruction at 4 mod 8: 4-byte ones only in pairs
        at += n
    assert head == HEAD, head
    code = [i for i in body if not i.endswith(":")]
    for n, i in enumerate(code):
        op = i.split()[0]
        if op.startswith("v_"):
            regs = vsrc(i) if op != "v_mov_b32_dpp" else []
            if len(regs) == 3:
                assert len({r & 1 for r in regs}) == 2, i                   # never three same-parity VGPR reads
            assert all(VGPR_LO <= r <= VGPR_HI for r in vsrc(i) + vdst(i)), i
        if op.startswith("v_rsq"):                                          # a wait state between a transcendental and its consumer
            nxt = next(j for j in code[n + 1:] if j.startswith("v_"))
            assert vdst(i)[0] not in vsrc(nxt), (i, nxt)
        if op == "v_mov_b32_dpp":                                           # two wait states between a VALU write and a DPP read
            for j in code[max(0, n - 2):n]:
                assert not (set(vdst(j)) & set(vsrc(i))), (j, i)
        if op.startswith("global_store"):                                   # a wide store's data is not overwritten in the next two slots
            for j in code[n + 1:n + 3]:
                assert not (set(vdst(j)) & set(vsrc(i)[1:])), (i, j)
    one = step(A_BASE, 0)
    one = one[one.index("5:"):]
    valu = [i for i in one if i.startswith("v_")]
    pair = pairs()
    assert len(valu) == 249 and len(pair) == 240 and len([i for i in one if "_dpp" in i]) == 6
    assert len([i for i in pair if i.startswith("v_rsq_f32")]) == ROWS and len([i for i in pair if i.startswith("v_sub_f32")]) == 3 * ROWS
    assert len([i for i in pair if i.startswith("v_fma_f32") and ", -v" in i]) == 3 * ROWS
    return head


def main():
    ins = build()
    check(ins)
    vregs = ["v%d" % r for r in range(VGPR_LO, VGPR_HI + 1)]
    sregs = ["s%d" % r for r in range(PTR, SAVE + 2)]
    with open(OUT, "w") as f:
        f.write("// GENERATED by tools/gen_mutual_loop.py — do not edit.  See that file for the why.\n")
        f.write("#define NB_MUTUAL_LOOP \"%s\"\n" % "\\n\\t".join(ins))
        f.write("#define NB_MUTUAL_LOOP_CLOBBERS %s\n" % ", ".join('"%s"' % c for c in vregs + sregs + ["scc", "memory"]))
    one = step(A_BASE, 0)
    print("wrote %s (%d instructions, %d VALU per step, loop head %d bytes past a 64-byte line)"
          % (OUT, len([i for i in ins if not i.endswith(":")]), len([i for i in one[one.index("5:"):] if i.startswith("v_")]), HEAD))


if __name__ == "__main__":
    main()

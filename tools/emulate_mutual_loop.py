#!/usr/bin/env python3
"""Run the generated unit loop of the mutual pairing (tools/gen_mutual_loop.py) on a CPU model of one wave.

Not a model of timing and not bit-exact to the GPU (v_rsq_f32 and fma are computed through binary64 here): it executes the instruction text —
the scalar bookkeeping, the exec masks, the DPP shifts, the scalar loads and the vector stores with their addresses — so that what a unit
writes, where, and how often can be checked without a GPU (tests/test_mutual_loop_generated.py).  `model_unit` is the same arithmetic said
directly: per (row, source block) one chain of 1024 terms from zero, sources ascending; both go through fma() and rsq() below, so the two
agree bit for bit when the loop's control is right.  Every access is bounds-checked against the regions handed in.
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_mutual_loop as G   # noqa: E402

F32, F64, U32 = np.float32, np.float64, np.uint32
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
OPERANDS = {"src": "s[0:1]", "table": "s[2:3]", "a": "s4", "first": "s5", "count": "s6", "nb": "s7", "n": "s8", "d0": "s9", "lane": "v0"}


def fma(a, b, c):
    with np.errstate(all="ignore"):
        return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def rsq(x):
    with np.errstate(all="ignore"):
        return (1.0 / np.sqrt(x.astype(F64))).astype(F32)


class Wave:
    def __init__(self, regions):
        self.v = np.zeros((128, 64), F32)
        self.vu = self.v.view(U32)
        self.s = [0] * 104
        self.exec = M64
        self.mask = np.ones(64, bool)
        self.scc = 0
        self.regions = regions          # name -> (base address, uint32 array)
        self.writes = {}                # (region, dword index) -> times written
        self.steps = 0

    def set_exec(self, x):
        self.exec = x & M64
        self.mask = np.array([(self.exec >> l) & 1 for l in range(64)], bool)

    def find(self, addr, ndw):
        for name, (base, arr) in self.regions.items():
            if base <= addr and addr + 4 * ndw <= base + 4 * arr.size:
                assert (addr - base) % 4 == 0
                return name, arr, (addr - base) // 4
        raise AssertionError("access of %d dwords at 0x%x is outside every region" % (ndw, addr))


def sreg(tok):
    m = re.fullmatch(r"s(\d+)", tok)
    if m:
        return int(m.group(1)), 1
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", tok)
    return int(m.group(1)), int(m.group(2)) - int(m.group(1)) + 1


def sread(w, tok, width=1):
    if tok == "exec":
        return w.exec
    if tok[0] == "s":
        r, n = sreg(tok)
        assert n == width, tok
        return w.s[r] if n == 1 else w.s[r] | (w.s[r + 1] << 32)
    x = int(tok, 0)
    return x & (M32 if width == 1 else M64)


def swrite(w, tok, x, width=1):
    if tok == "exec":
        w.set_exec(x)
        return
    r, n = sreg(tok)
    assert n == width, tok
    w.s[r] = x & M32
    if n == 2:
        w.s[r + 1] = (x >> 32) & M32


def vnum(tok):
    return int(re.fullmatch(r"-?v(\d+)", tok).group(1))


def vread(w, tok):
    """a 32-bit VALU source as 64 binary32 values"""
    if tok[0] == "-":
        return -w.v[vnum(tok)]
    if tok[0] == "v":
        return w.v[vnum(tok)]
    if tok[0] == "s":
        return np.full(64, sread(w, tok), U32).view(F32)
    return np.full(64, int(tok, 0) & M32, U32).view(F32)      # an integer inline constant or a literal: its bits


def vwrite(w, d, val):
    if w.exec == M64:
        w.v[d] = val
    else:
        np.copyto(w.v[d], val, where=w.mask)


def decode(ins):
    """instruction text -> list of callables f(w) returning the next pc or None"""
    code, labels = [], {}
    for i in ins:
        if i.endswith(":"):
            labels.setdefault(i[:-1], []).append(len(code))
        elif not i.startswith("."):
            code.append(i)

    def target(pc, t):
        name, way = t[:-1], t[-1]
        at = labels[name]
        return min(x for x in at if x > pc) if way == "f" else max(x for x in at if x <= pc)

    prog = []
    for pc, i in enumerate(code):
        op, rest = (i.split(None, 1) + [""])[:2]
        a = [x for x in re.split(r"[ ,]+", rest) if x]
        prog.append(make(op, a, pc, target, i))
    return prog


def make(op, a, pc, target, text):   # noqa: C901
    if op in ("s_nop", "s_waitcnt"):
        return lambda w: None
    if op in ("s_mov_b32", "s_movk_i32"):
        return lambda w: swrite(w, a[0], sread(w, a[1]))
    if op == "s_mov_b64":
        def f(w):
            x = sread(w, a[1], 2) if not re.fullmatch(r"-?\d+", a[1]) else int(a[1]) & M64
            swrite(w, a[0], x, 2)
        return f
    if op in ("s_add_u32", "s_addc_u32", "s_sub_u32", "s_subb_u32"):
        def f(w):
            x, y = sread(w, a[1]), sread(w, a[2])
            cin = w.scc if op in ("s_addc_u32", "s_subb_u32") else 0
            r = x + y + cin if op.startswith("s_add") else x - y - cin
            w.scc = int(r > M32 or r < 0)
            swrite(w, a[0], r & M32)
        return f
    if op == "s_lshl_b32":
        def f(w):
            r = (sread(w, a[1]) << (sread(w, a[2]) & 31)) & M32
            w.scc = int(r != 0)
            swrite(w, a[0], r)
        return f
    if op == "s_lshl_b64":
        def f(w):
            r = (sread(w, a[1], 2) << (sread(w, a[2]) & 63)) & M64
            w.scc = int(r != 0)
            swrite(w, a[0], r, 2)
        return f
    if op in ("s_mul_i32", "s_mul_hi_u32"):
        return lambda w: swrite(w, a[0], (sread(w, a[1]) * sread(w, a[2]) >> (32 if op == "s_mul_hi_u32" else 0)) & M32)
    if op.startswith("s_cmp_"):
        cmp = {"eq": lambda x, y: x == y, "lg": lambda x, y: x != y, "lt": lambda x, y: x < y, "ge": lambda x, y: x >= y}[op.split("_")[2]]
        assert op.endswith("_u32")

        def f(w):
            w.scc = int(cmp(sread(w, a[0]), sread(w, a[1])))
        return f
    if op in ("s_cselect_b32", "s_cselect_b64"):
        n = 2 if op.endswith("b64") else 1
        return lambda w: swrite(w, a[0], sread(w, a[1] if w.scc else a[2], n), n)
    if op in ("s_or_b32", "s_and_b64"):
        n = 2 if op.endswith("b64") else 1

        def f(w):
            x, y = sread(w, a[1], n), sread(w, a[2], n)
            r = x | y if op == "s_or_b32" else x & y
            w.scc = int(r != 0)
            swrite(w, a[0], r, n)
        return f
    if op == "s_branch":
        return lambda w: target(pc, a[0])
    if op in ("s_cbranch_scc0", "s_cbranch_scc1"):
        want = int(op[-1])
        return lambda w: target(pc, a[0]) if w.scc == want else None
    if op == "s_load_dwordx16":
        def f(w):
            r, n = sreg(a[0])
            assert n == 16
            _, arr, at = w.find(sread(w, a[1], 2) + int(a[2], 0), 16)
            w.s[r:r + 16] = [int(x) for x in arr[at:at + 16]]
        return f
    if op in ("global_load_dwordx4", "global_store_dwordx4"):
        load = op == "global_load_dwordx4"
        data, addr, base = (a[0], a[1], a[2]) if load else (a[1], a[0], a[2])
        off = int(a[3].split(":")[1]) if len(a) > 3 else 0
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", data)
        d0 = int(m.group(1))

        def f(w):
            for l in np.nonzero(w.mask)[0]:
                name, arr, at = w.find(sread(w, base, 2) + int(w.vu[vnum(addr), l]) + off, 4)
                if load:
                    w.vu[d0:d0 + 4, l] = arr[at:at + 4]
                else:
                    arr[at:at + 4] = w.vu[d0:d0 + 4, l]
                    for k in range(4):
                        w.writes[(name, at + k)] = w.writes.get((name, at + k), 0) + 1
        return f
    if op == "v_mov_b32_dpp":
        d, s = vnum(a[0]), vnum(a[1])
        assert "wave_shr:1" in text and "row_mask:0xf" in text and "bank_mask:0xf" in text
        bc = "bound_ctrl:1" in text

        def f(w):
            w.steps += 1
            src = np.empty(64, F32)
            src[1:] = w.v[s][:-1]
            valid = np.empty(64, bool)
            valid[1:] = w.mask[:-1]
            valid[0] = False
            src[0] = 0.0
            out = np.where(valid, src, F32(0.0) if bc else w.v[d])
            vwrite(w, d, out)
        return f
    if op in ("v_mov_b32_e32", "v_mov_b32_e64"):
        return lambda w: vwrite(w, vnum(a[0]), vread(w, a[1]))
    if op == "v_lshlrev_b32_e32":
        def f(w):
            vwrite(w, vnum(a[0]), ((vread(w, a[2]).view(U32).astype(np.uint64) << int(a[1])) & M32).astype(U32).view(F32))
        return f
    if op == "v_sub_f32_e64":
        return lambda w: vwrite(w, vnum(a[0]), vread(w, a[1]) - vread(w, a[2]))
    if op == "v_mul_f32_e64":
        return lambda w: vwrite(w, vnum(a[0]), vread(w, a[1]) * vread(w, a[2]))
    if op in ("v_fma_f32", "v_fmaak_f32"):
        return lambda w: vwrite(w, vnum(a[0]), fma(vread(w, a[1]), vread(w, a[2]), vread(w, a[3])))
    if op == "v_rsq_f32_e64":
        return lambda w: vwrite(w, vnum(a[0]), rsq(vread(w, a[1])))
    raise ValueError("no model of: " + text)


SRC_BASE, TABLE_BASE = 0x7F0000100000, 0x7F1000000000


def run_unit(pos, table, A, d0, count):
    """pos: (n, 4) float32, table: (nb, n, 4) float32, modified in place.  Returns {table dword index: times written}."""
    n = pos.shape[0]
    nb = n // 1024
    ins = [re.sub(r"%\[(\w+)\]", lambda m: OPERANDS[m.group(1)], i) for i in G.build()]
    prog = decode(ins)
    w = Wave({"src": (SRC_BASE, pos.view(U32).reshape(-1)), "table": (TABLE_BASE, table.view(U32).reshape(-1))})
    first = (A + d0) % nb
    for tok, x in (("s[0:1]", SRC_BASE), ("s[2:3]", TABLE_BASE)):
        swrite(w, tok, x, 2)
    for r, x in ((4, A), (5, first), (6, count), (7, nb), (8, n), (9, d0)):
        w.s[r] = x
    w.vu[0] = np.arange(64, dtype=U32)
    keep = list(w.s[:34]), w.vu[:8].copy()
    pc = 0
    with np.errstate(all="ignore"):
        while pc < len(prog):
            nxt = prog[pc](w)
            pc = pc + 1 if nxt is None else nxt
    assert w.exec == M64 and (list(w.s[:34]), True) == (keep[0], bool((w.vu[:8] == keep[1]).all())), "the loop changed a register it does not own"
    assert all(name == "table" for name, _ in w.writes)
    return {at: c for (_, at), c in w.writes.items()}, w.steps // 6


def model_unit(pos, A, d0, count):
    """{(table block, row): (fx, fy, fz)} of what the unit leaves in the table"""
    n = pos.shape[0]
    nb = n // 1024
    eps = np.array([G.SOFT_BITS], U32).view(F32)[0]
    rows = pos[1024 * A:1024 * A + 1024, :3]
    out = {}
    with np.errstate(all="ignore"):
        for k in range(count):
            b = (A + d0 + k) % nb
            srcs = pos[1024 * b:1024 * b + 1024, :3]
            for mirrored in ((False, True) if d0 else (False,)):
                own, other = (srcs, rows) if mirrored else (rows, srcs)      # own: the rows that accumulate; other: what they meet, ascending
                acc = np.zeros((1024, 3), F32)
                for j in range(1024):
                    d = own - other[j] if mirrored else other[j] - own          # source - row, as the loop forms it
                    d2 = fma(d[:, 0], d[:, 0], fma(d[:, 1], d[:, 1], fma(d[:, 2], d[:, 2], np.full(1024, eps, F32))))
                    inv = rsq(d2)
                    inv3 = inv * (inv * inv)
                    if mirrored:
                        d = -d                                                   # the operand modifier
                    for c in range(3):
                        acc[:, c] = fma(d[:, c], inv3, acc[:, c])
                base_row = 1024 * (b if mirrored else A)
                blk = A if mirrored else b
                for r in range(1024):
                    out[(blk, base_row + r)] = acc[r].copy()
    return out


if __name__ == "__main__":
    nb_, A_, d0_, count_ = (int(x) for x in sys.argv[1:5])
    rng = np.random.default_rng(1)
    p = rng.standard_normal((1024 * nb_, 4)).astype(F32)
    t = np.full((nb_, 1024 * nb_, 4), np.nan, F32)
    wr, steps = run_unit(p, t, A_, d0_, count_)
    want = model_unit(p, A_, d0_, count_)
    bad = sum(1 for (blk, row), f in want.items() if not np.array_equal(t[blk, row, :3].view(U32), f.view(U32)) or t[blk, row, 3] != 0)
    print("steps %d, dwords written %d (max %d times), words expected %d, words that differ %d" % (steps, len(wr), max(wr.values()), len(want), bad))

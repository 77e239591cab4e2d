"""The generated unit loop of the mutual pairing (tools/gen_mutual_loop.py -> mini_nbody_amd/csrc/mutual_loop_gfx950.inc):
the committed text is the generator's, the rules it is built on hold ON THE EMITTED TEXT (read back from the include, not taken from the
generator's own lists), and the loop's control — masks, shifts, block bookkeeping, every address — writes exactly the words a unit owns
(tools/emulate_mutual_loop.py: one wave on a CPU model, every access bounds-checked).  No GPU."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "mini_nbody_amd", "csrc", "mutual_loop_gfx950.inc")


def tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gen():
    return tool("gen_mutual_loop")


@pytest.fixture(scope="module")
def text():
    """the instructions of NB_MUTUAL_LOOP as committed, labels and directives included"""
    with open(INC) as f:
        src = f.read()
    m = re.search(r'#define NB_MUTUAL_LOOP "(.*)"\n', src)
    return m.group(1).split("\\n\\t")


@pytest.fixture(scope="module")
def steps(text):
    """the eight steps of the inner loop, each from its first shift to its lane-63 store: lists of instructions"""
    loop = text[text.index("1:"):]
    loop = loop[:loop.index("s_cbranch_scc1 1b")]
    out, cur = [], None
    for n, i in enumerate(loop):
        if "_dpp" in i and "_dpp" not in loop[n - 1]:
            cur = []
        if cur is not None:
            cur.append(i)
            if i.startswith("global_store_dwordx4 v111"):
                out.append(cur)
                cur = None
    assert len(out) == 8
    return out


def vregs(i):
    return [int(x) for x in re.findall(r"\bv(\d+)\b", i)] + [int(x) for m in re.findall(r"v\[(\d+):(\d+)\]", i) for x in m]


def reads(i):
    """VGPRs a VALU instruction reads: all but the destination; a DPP move reads its destination too (`old`)"""
    r = [int(x) for x in re.findall(r"\bv(\d+)\b", i)]
    return r if "_dpp" in i else r[1:]


def test_committed_text_is_the_generators(gen, tmp_path, monkeypatch):
    out = tmp_path / "mutual_loop_gfx950.inc"
    monkeypatch.setattr(gen, "OUT", str(out))
    gen.main()
    with open(INC, "rb") as f:
        assert out.read_bytes() == f.read(), "regenerate: python3 tools/gen_mutual_loop.py, then make lib"


def size(i):
    op = i.split()[0]
    if i.endswith(":"):
        return 0
    if op.startswith("v_") or op.startswith("global_") or op.startswith("s_load"):
        return 8
    assert op.startswith("s_") and not re.search(r"0x[0-9a-f]{5,}", i), i      # scalar, no 32-bit literal
    return 4


def test_every_instruction_is_eight_bytes_at_four_mod_eight(text):
    body = text[text.index(".p2align 6") + 1:]
    at, head, n8 = 0, None, 0
    for i in body:
        if i == "1:":
            head = at % 64
        if size(i) == 8:
            n8 += 1
            assert at % 8 == 4, "%s starts at %d mod 8" % (i, at % 8)
            op = i.split()[0]      # the 8-byte forms: VOP3, VOP2 with a literal, DPP, global, s_load
            assert not op.startswith("v_") or op.endswith("_e64") or op in ("v_fma_f32", "v_fmaak_f32", "v_mov_b32_dpp"), i
        at += size(i)
    assert head == 60 and n8 > 8 * 249      # the loop head's fixed offset past a 64-byte line
    assert not any(i.startswith(".") for i in body)


def test_no_three_vgpr_reads_of_one_parity(text):
    body = text[text.index(".p2align 6") + 1:]
    n3 = 0
    for i in body:
        if i.startswith("v_") and "_dpp" not in i and len(reads(i)) == 3:
            n3 += 1
            assert len({r & 1 for r in reads(i)}) == 2, i
    assert n3 == 8 * (32 + 96)      # per step: two d2 fma per row, six accumulating fma per row


def test_wait_states(text):
    code = [i for i in text[text.index(".p2align 6") + 1:] if not i.endswith(":")]
    nrsq = 0
    for n, i in enumerate(code):
        if i.startswith("v_rsq_f32"):
            nrsq += 1
            dst = vregs(i)[0]
            later = [j for j in code[n + 1:] if j.startswith("v_")]
            first = next(k for k, j in enumerate(later) if dst in reads(j))
            assert first >= 1, (i, later[0])                              # its result is first read at least one VALU instruction later
        if "_dpp" in i:                                                   # a VALU-written VGPR is read by DPP two slots later at the earliest
            for j in code[n - 2:n]:
                assert not (j.startswith("v_") and vregs(j)[0] in reads(i)), (j, i)
        if i.startswith("global_store_dwordx4"):                          # a wide store's data is not overwritten in the next two slots
            data = set(range(*[int(x) + k for k, x in enumerate(re.search(r"v\[(\d+):(\d+)\]", i).groups())]))
            for j in code[n + 1:n + 3]:
                assert not (j.startswith("v_") and vregs(j)[0] in data), (i, j)
    assert nrsq == 8 * 16
    # nothing outside this list: no exec write by the VALU, no lane access, no LDS, no AGPR; memory is read by the scalar unit (and the
    # prologue's loads of the lane's rows) and written by vector stores
    allowed = {"s_mov_b32", "s_mov_b64", "s_movk_i32", "s_add_u32", "s_addc_u32", "s_sub_u32", "s_subb_u32", "s_lshl_b32", "s_lshl_b64", "s_mul_i32",
               "s_mul_hi_u32", "s_cmp_eq_u32", "s_cmp_lg_u32", "s_cmp_lt_u32", "s_cmp_ge_u32", "s_cselect_b32", "s_cselect_b64", "s_or_b32", "s_and_b64",
               "s_branch", "s_cbranch_scc0", "s_cbranch_scc1", "s_nop", "s_waitcnt", "s_load_dwordx16", "global_load_dwordx4", "global_store_dwordx4",
               "v_mov_b32_dpp", "v_mov_b32_e32", "v_mov_b32_e64", "v_lshlrev_b32_e32", "v_sub_f32_e64", "v_mul_f32_e64", "v_fma_f32", "v_fmaak_f32",
               "v_rsq_f32_e64"}
    ops = {i.split()[0] for i in text if not i.endswith(":") and not i.startswith(".")}
    assert ops <= allowed, ops - allowed
    assert not any(i.startswith("global_load") for i in code)           # the loop itself loads through the scalar unit only


def test_counts_per_step(steps):
    for st in steps:
        valu = [i for i in st if i.startswith("v_")]
        shifts = [i for i in valu if "_dpp" in i]
        assert len(shifts) == 6 and all("wave_shr:1 row_mask:0xf bank_mask:0xf" in i for i in shifts)
        pair = [i for i in valu if "_dpp" not in i and not i.startswith("v_mov_b32")]
        assert len(pair) == 240 and len(valu) == 240 + 6 + 3
        assert len([i for i in pair if i.startswith("v_rsq_f32")]) == 16
        assert len([i for i in pair if i.startswith("v_sub_f32")]) == 48
        assert len([i for i in pair if i.startswith("v_fmaak_f32")]) == 16 and len([i for i in pair if i.startswith("v_mul_f32")]) == 32
        fma = [i for i in pair if i.startswith("v_fma_f32")]
        mirrored = [i for i in fma if ", -v" in i]
        direct = [i for i in fma if ", -v" not in i and 56 <= vregs(i)[0] < 104]
        assert len(mirrored) == 48 and len(direct) == 48 and len(fma) == 48 + 48 + 32
        assert all(108 <= vregs(i)[0] <= 110 and vregs(i)[0] == vregs(i)[3] for i in mirrored)
        assert all(vregs(i)[0] == vregs(i)[3] for i in direct)


def test_rows_ascend_in_both_chains(steps):
    for st in steps:
        # the row of an accumulating fma is known by the row of the subtraction that last wrote its difference register
        owner, direct, mirrored = {}, [], []
        for i in st:
            if i.startswith("v_sub_f32"):
                d, _, pos = vregs(i)
                owner[d] = (pos - 8) % 16
            elif i.startswith("v_fma_f32") and ", -v" in i:
                mirrored.append((owner[vregs(i)[1]], vregs(i)[0] - 108))
            elif i.startswith("v_fma_f32") and 56 <= vregs(i)[0] < 104:
                direct.append((owner[vregs(i)[1]], (vregs(i)[0] - 56) // 16))
                assert (vregs(i)[0] - 56) % 16 == owner[vregs(i)[1]], i          # row r's difference feeds row r's accumulator
        want = [(r, c) for r in range(16) for c in range(3)]
        assert direct == want and mirrored == want


def test_registers(text, gen):
    used = [r for i in text for r in vregs(i)]
    assert max(used) < 128 and min(used) >= 8
    with open(INC) as f:
        clob = re.search(r"#define NB_MUTUAL_LOOP_CLOBBERS (.*)\n", f.read()).group(1)
    named = set(re.findall(r'"(\w+)"', clob))
    assert {"v%d" % r for r in used} <= named
    sused = {int(x) for i in text for x in re.findall(r"\bs(\d+)\b", i)} | \
            {r for i in text for a, b in re.findall(r"s\[(\d+):(\d+)\]", i) for r in range(int(a), int(b) + 1)}
    assert {"s%d" % r for r in sused} <= named and max(sused) < 100 and "memory" in named and "scc" in named


UNITS = [(2, 0, 1, 1),    # the half offset at nb = 2: one partner block
         (2, 1, 0, 1),    # a diagonal unit: the mirrored sums never stored
         (5, 4, 1, 2)]    # two partner blocks that wrap past nb: the flush and the lane-63 address at a block boundary


@pytest.mark.parametrize("nb,a,d0,count", UNITS)
def test_a_unit_writes_its_words_once_and_right(nb, a, d0, count):
    emu = tool("emulate_mutual_loop")
    rng = np.random.default_rng(nb * 100 + a)
    pos = rng.standard_normal((1024 * nb, 4)).astype(np.float32)
    pos[7, :3] = pos[1024 * ((a + d0) % nb) + 1023, :3]                 # a coincident pair across the array's ends
    table = np.full((nb, 1024 * nb, 4), np.nan, np.float32)
    writes, nsteps = emu.run_unit(pos, table, a, d0, count)
    want = emu.model_unit(pos, a, d0, count)
    assert nsteps == 1024 * count + 64
    assert len(want) == 1024 * count * (2 if d0 else 1)
    words = {at // 4 for at in writes}
    assert words == {blk * 1024 * nb + row for blk, row in want} and set(writes.values()) == {1} and len(writes) == 4 * len(want)
    for (blk, row), f in want.items():
        got = table[blk, row]
        assert np.array_equal(got[:3].view(np.uint32), f.view(np.uint32)) and got.view(np.uint32)[3] == 0, (blk, row)

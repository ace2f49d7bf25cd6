"""DPP read-hazard lint of the generated gfx950 code (CPU only: hipcc cross-compiles, llvm-objdump disassembles).

The hardware does not interlock a DPP read of a VGPR that a VALU instruction wrote less than two wait states before
(CDNA3 / CDNA4 ISA guide, "Manually inserted wait states": VALU writes VGPR -> v_*_dpp reads that VGPR as its DPP
operand: 2).  LLVM's hazard recogniser inserts the `s_nop` for instructions it schedules itself, but the row-broadcast
multiply-adds of csrc/mpcqp_devwave.h (chain4, rowbc_fms, fmabc4) are inline assembly: the compiler neither looks inside
a block nor keeps a VALU write of one of its operands away from its first instruction.  The blocks carry their own
`s_nop 1`; this lint checks that every DPP instruction of the shipped code objects and of the largest team
specialisations really has its two wait states.

Wait states are counted as the ISA guide does: `s_nop N` is N + 1, every other instruction is 1.  64-bit operands are
register pairs.  A branch is followed to its target (the taken edge) as well as through (fall-through)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
NEED = 2                      # wait states between the VALU write and the DPP read

_REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
_DPP_CTRL = ("quad_perm:", "row_shl:", "row_shr:", "row_ror:", "row_mirror", "row_half_mirror", "row_bcast:", "row_newbcast:",
             "wave_shl", "wave_shr", "wave_rol", "wave_ror", "row_share:", "row_xmask:", "dpp8:")
_ENDS = ("s_branch", "s_endpgm", "s_setpc_b64", "s_swappc_b64", "s_trap")


def _vregs(tok):
    """VGPR numbers named by one operand token ('v3', '-v[6:7]', '|v2|', 's[0:1]', 'vcc', '0x10' ...)."""
    out = set()
    for m in _REG.finditer(tok):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


class Inst:
    __slots__ = ("op", "text", "addr", "ops", "is_dpp", "dpp_reads", "valu_writes", "states", "target", "ends", "func")

    def __init__(self, text, addr, func):
        self.text, self.addr, self.func = text, addr, func
        parts = text.split(None, 1)
        self.op = parts[0]
        rest = parts[1] if len(parts) > 1 else ""
        # operands: comma separated; modifiers (row_newbcast:3 row_mask:0xf, op_sel:[0,1] ...) follow the last one after a blank
        self.ops = [p.strip().split()[0] for p in rest.split(",") if p.strip()] if rest else []
        self.is_dpp = self.op.endswith("_dpp") or any(c in rest for c in _DPP_CTRL)
        # the operand that goes through the DPP path is src0: the first operand after the destination
        self.dpp_reads = _vregs(self.ops[1]) if self.is_dpp and len(self.ops) > 1 else set()
        self.valu_writes = set()
        if self.op.startswith("v_") and self.ops and not self.op.startswith(("v_nop", "v_cmpx")):
            self.valu_writes = _vregs(self.ops[0])
            if self.op.startswith("v_swap") and len(self.ops) > 1:
                self.valu_writes |= _vregs(self.ops[1])
        self.states = 1
        if self.op == "s_nop":
            self.states = int(self.ops[0], 0) + 1
        self.ends = self.op.startswith(_ENDS)
        self.target = None
        if self.op.startswith(("s_cbranch", "s_branch")) and self.ops and addr is not None:
            try:
                imm = int(self.ops[0], 0) & 0xFFFF
                self.target = addr + 4 + 4 * (imm - 0x10000 if imm & 0x8000 else imm)
            except ValueError:
                pass


def parse_listing(text):
    """Instructions of an `llvm-objdump -d` listing (or of plain assembly text: no addresses, no branch following)."""
    insts, func = [], None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <(.+)>:\s*$", line)
        if m:
            func = m.group(1)
            continue
        code, _, comment = line.partition("//")
        code = code.split(";", 1)[0].strip()
        if not code or code.endswith(":") or code.startswith((".", "Disassembly", "/")) or "file format" in code:
            continue
        am = re.match(r"\s*([0-9a-fA-F]+):", comment)
        insts.append(Inst(code, int(am.group(1), 16) if am else None, func))
    return insts


def find_dpp_hazards(insts, need=NEED):
    """[(writer, dpp instruction, wait states between them)] for every DPP instruction that reads, through the DPP path,
    a VGPR some VALU instruction wrote fewer than `need` wait states earlier -- along the layout order and along taken
    branches."""
    by_addr = {i.addr: k for k, i in enumerate(insts) if i.addr is not None}
    found = []

    def check_from(k, pending):
        # pending: [(writer, wait states already passed since it)]; walk forward while any writer is still inside the window
        while pending and k < len(insts):
            ins = insts[k]
            if ins.is_dpp:
                for wr, gone in pending:
                    if gone < need and wr.valu_writes & ins.dpp_reads:
                        found.append((wr, ins, gone))
            pending = [(wr, gone + ins.states) for wr, gone in pending if gone + ins.states < need]
            if ins.target is not None and pending and ins.target in by_addr:
                check_from(by_addr[ins.target], list(pending))
            if ins.ends:
                return
            k += 1

    for k, ins in enumerate(insts):
        if ins.valu_writes:
            check_from(k + 1, [(ins, 0)])
    # one entry per (writer, reader) pair
    seen, out = set(), []
    for wr, rd, gone in found:
        if (id(wr), id(rd)) not in seen:
            seen.add((id(wr), id(rd)))
            out.append((wr, rd, gone))
    return out


def describe(hazards, limit=8):
    return "\n".join(f"  {rd.func}: `{wr.text}` -> `{rd.text}` ({gone} wait state(s) between, {NEED} needed)"
                     + (f" at 0x{rd.addr:x}" if rd.addr is not None else "") for wr, rd, gone in hazards[:limit])


# ---- the checker on hand-written listings: it can fail -----------------------------------------------------------------------
VIOLATION = """
0000000000001600 <kernel_a>:
	v_add_f64 v[2:3], v[0:1], v[0:1]                           // 000000001648: D2800002 00020100
	v_fmac_f64_dpp v[0:1], v[2:3], v[0:1] row_newbcast:3 row_mask:0xf bank_mask:0xf// 000000001650: 080000FA FF015302
"""
WITH_NOP = """
0000000000001600 <kernel_b>:
	v_add_f64 v[2:3], v[0:1], v[0:1]                           // 000000001648: D2800002 00020100
	s_nop 1                                                    // 000000001650: BF800001
	v_fmac_f64_dpp v[0:1], v[2:3], v[0:1] row_newbcast:3 row_mask:0xf bank_mask:0xf// 000000001654: 080000FA FF015302
"""
TWO_INDEPENDENT = """
0000000000001600 <kernel_c>:
	v_add_f64 v[2:3], v[0:1], v[0:1]                           // 000000001648: D2800002 00020100
	v_lshlrev_b32_e32 v5, 2, v9                                // 000000001650: 240A0482
	s_waitcnt vmcnt(0)                                         // 000000001654: BF8C0F70
	v_fmac_f64_dpp v[0:1], v[2:3], v[0:1] row_newbcast:3 row_mask:0xf bank_mask:0xf// 000000001658: 080000FA FF015302
"""
PAIR_OVERLAP = """
0000000000001600 <kernel_d>:
	v_mov_b32_e32 v3, v7                                       // 000000001648: 7E060307
	v_xor_b32_e32 v9, 1, v8                                    // 00000000164C: 2A060481
	v_fmac_f64_dpp v[0:1], -v[2:3], v[4:5] row_newbcast:15 row_mask:0xf bank_mask:0xf// 000000001650: 080000FA FF015302
"""


def test_lint_reports_a_dpp_read_right_behind_the_valu_write():
    hz = find_dpp_hazards(parse_listing(VIOLATION))
    assert len(hz) == 1 and hz[0][0].op == "v_add_f64" and hz[0][1].op == "v_fmac_f64_dpp" and hz[0][2] == 0
    assert "kernel_a" in describe(hz)


def test_lint_accepts_s_nop_1_between_write_and_dpp_read():
    assert find_dpp_hazards(parse_listing(WITH_NOP)) == []
    # s_nop 0 is one wait state only
    hz = find_dpp_hazards(parse_listing(WITH_NOP.replace("s_nop 1", "s_nop 0")))
    assert len(hz) == 1 and hz[0][2] == 1


def test_lint_accepts_two_independent_instructions_between():
    assert find_dpp_hazards(parse_listing(TWO_INDEPENDENT)) == []
    one = TWO_INDEPENDENT.replace("\ts_waitcnt vmcnt(0)                                         // 000000001654: BF8C0F70\n", "")
    assert len(find_dpp_hazards(parse_listing(one))) == 1


def test_lint_treats_64_bit_operands_as_register_pairs():
    # v3 is the high half of the DPP operand v[2:3] (negated: the modifier does not hide it); one instruction between
    hz = find_dpp_hazards(parse_listing(PAIR_OVERLAP))
    assert len(hz) == 1 and hz[0][0].text.startswith("v_mov_b32_e32 v3") and hz[0][2] == 1
    # the write of v9 is no hazard, nor a write of the NON-DPP operands (v[4:5] is src1, v[0:1] the accumulator)
    assert find_dpp_hazards(parse_listing(PAIR_OVERLAP.replace("v_mov_b32_e32 v3, v7", "v_mov_b32_e32 v5, v7"))) == []
    assert find_dpp_hazards(parse_listing(PAIR_OVERLAP.replace("v_mov_b32_e32 v3, v7", "v_mov_b32_e32 v1, v7"))) == []


def test_lint_follows_taken_branches_and_stops_at_unconditional_ones():
    taken = """
0000000000001000 <kernel_e>:
	v_mul_f64 v[2:3], v[0:1], v[0:1]                           // 000000001000: D2810002 00020100
	s_cbranch_scc1 2                                           // 000000001008: BF850002
	s_nop 1                                                    // 00000000100C: BF800001
	s_nop 1                                                    // 000000001010: BF800001
	v_fmac_f64_dpp v[0:1], v[2:3], v[0:1] row_newbcast:3 row_mask:0xf bank_mask:0xf// 000000001014: 080000FA FF015302
"""
    hz = find_dpp_hazards(parse_listing(taken))          # the branch itself is the only wait state on the taken edge
    assert len(hz) == 1 and hz[0][2] == 1
    dead = taken.replace("s_cbranch_scc1 2 ", "s_branch 65535 ").replace("\ts_nop 1                                                    // 00000000100C: BF800001\n", "").replace(
        "\ts_nop 1                                                    // 000000001010: BF800001\n", "")
    assert find_dpp_hazards(parse_listing(dead)) == []   # (what follows an unconditional branch in the layout does not follow it in time)


# ---- the real code ---------------------------------------------------------------------------------------------------------
def disassemble_device_code(so, workdir):
    """Disassembly of every gfx950 code object bundled in the shared object `so` (a copy under `workdir` is unbundled:
    llvm-objdump --offloading writes next to its input).  Returns [(code object path, listing text)]."""
    from tests.team_util import device_code_objects
    out = []
    for co in device_code_objects(so, workdir):
        r = subprocess.run([OBJDUMP, "-d", co], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append((co, r.stdout))
    return out


def _lint_shared_object(so, workdir, must_have_dpp=True):
    n_dpp, hazards = 0, []
    for co, text in disassemble_device_code(so, workdir):
        insts = parse_listing(text)
        n_dpp += sum(1 for i in insts if i.is_dpp)
        hazards += find_dpp_hazards(insts)
    if must_have_dpp:
        assert n_dpp > 0, f"no DPP instruction found in {so}: the lint looks at nothing"
    assert not hazards, f"{len(hazards)} DPP read hazard(s) in {os.path.basename(so)}:\n" + describe(hazards)
    return n_dpp


@pytest.mark.slow
def test_library_code_objects_have_no_dpp_read_hazard(tmp_path):
    """libmpcqp.so: the ahead-of-time step kernels, the runtime-dimension kernel, the MHE / small-problem / stage kernels."""
    import mpcqp
    mpcqp.load_library()
    so = os.path.join(ROOT, "modelpredictivecontrol.jl_amd", "lib", "libmpcqp.so")
    assert _lint_shared_object(so, str(tmp_path)) > 100


# nZ̃ = 151 (12,3,3,50,50, C3 pattern) and 141 (12,2,2,70,70, pattern "all"): three rows per lane, the DPP row chains of
# chol_big_panel_* and the big substitutions -- on a team of four (the product default there) and of two
@pytest.mark.slow
@pytest.mark.parametrize("case,team", [("plain151", 4), ("plain141", 4), ("plain151", 2), ("plain141", 2)])
def test_team_specialisations_have_no_dpp_read_hazard(case, team, tmp_path):
    from tests import team_util as tu
    cache = tmp_path / "cache"
    cache.mkdir(mode=0o700)
    so = tu.prebuild_plain(case, team, str(cache))
    syms = tu.kernel_symbols(so, str(tmp_path / "syms"))
    assert tu.team_of_symbols(syms) == team, syms
    assert _lint_shared_object(so, str(tmp_path / "dis")) > 100

"""scripts/loop_waits.py on a hand-written assembly fragment: kernel naming,
the step loop as the largest backward-branch extent, and the exposed-round-trip
count (a batch of reads ahead of one full wait counts once; a read followed by
a counted wait or by further LDS instructions does not count)."""
import importlib.util
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent

ASM = """\
\t.text
_ZN12_GLOBAL__N_110env_kernelILi8ELb0ELb1ELb0ELi2ELb0EEEvNS_6ParamsE: ; @kernel
\tds_read_b32 v0, v1
\ts_waitcnt lgkmcnt(0)
.LBB0_1:
\t.loc\t0 10 5                        ; voxnav_env.hip:10:5 @[ voxnav_env.hip:100:9 ]
\tds_read_b64 v[0:1], v2
\tds_read_b64 v[2:3], v3
\ts_waitcnt lgkmcnt(0)
.LBB0_2:
\t.loc\t0 20 5                        ; voxnav_env.hip:20:5
\tds_read_b32 v4, v5
\ts_waitcnt vmcnt(0)
\ts_waitcnt lgkmcnt(0)
\ts_cbranch_scc1 .LBB0_2
\tds_read_b32 v6, v7
\tds_read_b32 v8, v9
\ts_waitcnt lgkmcnt(1)
\tglobal_store_dwordx4 v[10:11], v[12:15], off
\ts_waitcnt lgkmcnt(0)
\tds_read_b32 v6, v7
\tds_write_b32 v7, v6
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\ts_branch .LBB0_1
\tds_read_b32 v0, v1
\ts_waitcnt lgkmcnt(0)
\ts_endpgm
.Lfunc_end0:
"""


def load():
    spec = importlib.util.spec_from_file_location("loop_waits", REPO / "scripts" / "loop_waits.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_kernel_names():
    lw = load()
    assert lw.mangled("env_kernel<8,false,true,false,2>") == "10env_kernelILi8ELb0ELb1ELb0ELi2ELb0EE"
    assert lw.mangled("env_kernel<16, false, true, false, 3, true>") == "10env_kernelILi16ELb0ELb1ELb0ELi3ELb1EE"
    assert lw.mangled("ILi8ELb0") == "ILi8ELb0"


def test_loop_extent_sequence_and_exposed_reads():
    lw = load()
    lines = ASM.splitlines()
    s, e = lw.function_lines(lines, lw.mangled("env_kernel<8,false,true,false,2>"))
    lo, hi = lw.loop_extent(lines, s, e)
    assert lines[lo].startswith(".LBB0_1:") and lines[hi].strip() == "s_branch .LBB0_1"   # not the inner .LBB0_2 loop
    seq = lw.sequence(lines, lo, hi)
    assert [k for k, _, _ in seq] == list("LLWLWWLLWVWLLW")      # the reads before and after the loop are outside
    assert seq[0][2] == "voxnav_env.hip:10 < voxnav_env.hip:100"
    exp = lw.exposed(seq)
    # the pair's second read and the lone read (a vmcnt-only wait between does not end the search);
    # not the reads ahead of lgkmcnt(1), and not the read followed by an LDS write
    assert [seq[i][1] for i in exp] == ["ds_read_b64 v[2:3], v3", "ds_read_b32 v4, v5"]

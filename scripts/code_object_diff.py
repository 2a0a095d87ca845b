#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libvoxnav.so, for changes
that must leave the kernels alone (host-side refactors).

Per library: the code objects (scripts/isa_check.py ``code_objects``), one per
translation unit, each with its kernel symbols (``*.kd``), its other defined
objects (``c_mt_g`` and the like) and a hash of ``.text``.  Units are matched
by their kernel sets.  Exit status 0 when both libraries hold the same kernel
symbols and every unit with kernels has a byte-identical ``.text``.

A unit whose hash differs gets a per-function report (``functions``): every
function symbol of ``.text`` is "identical" when its size and its disassembly
agree with addresses dropped and the literal of the PC-relative add after
``s_getpc_b64`` masked (that literal, the distance to the unit's constant
tables or to a callee, shifts with any size change elsewhere in the unit).

A unit that gained or lost kernels has no unit with the same kernel set; it is
paired with the new unit that shares the most kernel names and gets the same
per-function report (``paired: "by overlap"``).  ``--rename OLD=NEW`` (any
number) rewrites function names of the old build before names are compared,
for a kernel whose mangled name changed and whose code should not have (a
template that gained a defaulted-false parameter: ``EEEvNS_6BcArgsE=ELb0EEEvNS_6BcArgsE``).

  python scripts/code_object_diff.py old/libvoxnav.so new/libvoxnav.so [--rename OLD=NEW ...]
"""
from __future__ import annotations

import hashlib
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from isa_check import code_objects  # noqa: E402

LLVM = Path("/opt/rocm/llvm/bin")


def units(so: Path):
    out = []
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(code_objects(so)):
            f = Path(td) / f"co{k}.elf"
            f.write_bytes(co)
            tab = subprocess.run([str(LLVM / "llvm-objdump"), "-t", str(f)], capture_output=True, text=True,
                                 check=True).stdout
            syms = [ln.split()[-1] for ln in tab.splitlines()
                    if ln[:1] in "0123456789abcdef" and ln.strip() and "*UND*" not in ln and " df " not in ln
                    and len(ln.split()) >= 4 and not ln.split()[-1].startswith(".")]
            text = Path(td) / f"co{k}.text"
            subprocess.run([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=.text", str(f), str(text)],
                           check=True)
            blob = text.read_bytes() if text.exists() else b""
            kernels = frozenset(s[:-3] for s in syms if s.endswith(".kd"))
            # (__hip_cuid_*: the unit's id, a hash of its path and options)
            objects = sorted(s for s in syms if not s.endswith(".kd") and s not in kernels
                             and not s.startswith("__hip_cuid_"))
            out.append({"kernels": kernels, "objects": objects, "text_bytes": len(blob),
                        "text_sha256": hashlib.sha256(blob).hexdigest(), "elf": co})
    return out


def functions(elf: bytes):
    """{function symbol of .text: (size, instructions without addresses and PC-relative literals)}"""
    with tempfile.TemporaryDirectory() as td:
        f = Path(td) / "co.elf"
        f.write_bytes(elf)
        objdump = [str(LLVM / "llvm-objdump"), "--no-show-raw-insn", "--no-leading-addr"]
        tab = subprocess.run([*objdump, "-t", str(f)], capture_output=True, text=True, check=True).stdout
        dis = subprocess.run([*objdump, "-d", str(f)], capture_output=True, text=True, check=True).stdout
    size = {ln.split()[-1]: int(ln.split(".text")[1].split()[0], 16) for ln in tab.splitlines() if " F .text" in ln}
    out, cur, pc = {}, None, 0
    for ln in dis.splitlines():
        head = re.match(r"^[0-9a-f]* ?<(.+)>:$", ln)
        if head:
            cur = out.setdefault(head.group(1), []) if head.group(1) in size else None
            continue
        ins = ln.split("//")[0].strip()
        # "...": objdump's elision of the zero padding up to the next function's
        # alignment, outside the symbol's size; the unit's last function has none
        if cur is None or not ins or ins == "...":
            continue
        # s_getpc_b64, then s_add_u32 / s_addc_u32 with the literal
        pc = 2 if ins.startswith("s_getpc_b64") else pc - 1
        if pc in (0, 1) and ins.startswith(("s_add_u32", "s_addc_u32")):
            ins = ins.rsplit(",", 1)[0] + ", <pcrel>"
        cur.append(ins)
    return {k: (size[k], v) for k, v in out.items()}


def renamed(name: str, renames) -> str:
    for old, new in renames:
        name = name.replace(old, new)
    return name


def function_report(old: bytes, new: bytes, renames=()):
    a, b = functions(old), functions(new)
    a = {renamed(k, renames): v for k, v in a.items()}
    rep = {"identical": sorted(k for k in a if a[k] == b.get(k)), "changed": {}, "only_old": sorted(set(a) - set(b)),
           "only_new": sorted(set(b) - set(a))}
    for k in sorted(set(a) & set(b)):
        if a[k] != b[k]:
            rep["changed"][k] = {"bytes": [a[k][0], b[k][0]], "instructions": [len(a[k][1]), len(b[k][1])]}
    return rep


def main(old: Path, new: Path, renames=()) -> int:
    a, b = units(old), units(new)
    ka = {k for u in a for k in u["kernels"]}
    kb = {k for u in b for k in u["kernels"]}
    rep = {"code_objects": [len(a), len(b)], "kernels": [len(ka), len(kb)], "only_old": sorted(ka - kb), "only_new": sorted(kb - ka), "units": []}
    ok = ka == kb
    by_set = {u["kernels"]: u for u in b}
    for u in a:
        v = by_set.get(u["kernels"])
        same = v is not None and v["text_sha256"] == u["text_sha256"] and v["objects"] == u["objects"]
        ok = ok and (same or not u["kernels"])
        rep["units"].append({"kernels": len(u["kernels"]), "text_bytes": u["text_bytes"], "identical": same})
        if v is None and u["kernels"]:
            names = {renamed(k, renames) for k in u["kernels"]}
            v = max(b, key=lambda w: len(names & w["kernels"]))
            if not names & v["kernels"]:
                continue
            rep["units"][-1]["paired"] = "by overlap"
        if v is not None and v["text_sha256"] != u["text_sha256"]:
            rep["units"][-1].update(text_bytes_new=v["text_bytes"],
                                    functions=function_report(u["elf"], v["elf"], renames))
    rep["kernel_free_units_new"] = [{"text_bytes": u["text_bytes"], "objects": u["objects"]}
                                    for u in b if not u["kernels"]]
    rep["ok"] = ok
    print(json.dumps(rep, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    pairs = [tuple(sys.argv[k + 1].split("=", 1)) for k, w in enumerate(sys.argv) if w == "--rename"]
    sys.exit(main(Path(sys.argv[1]), Path(sys.argv[2]), pairs))

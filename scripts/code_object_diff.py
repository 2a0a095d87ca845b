#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libvoxnav.so, for changes
that must leave the kernels alone (host-side refactors).

Per library: the code objects (scripts/isa_check.py ``code_objects``), one per
translation unit, each with its kernel symbols (``*.kd``), its other defined
objects (``c_mt_g`` and the like) and a hash of ``.text``.  Units are matched
by their kernel sets.  Exit status 0 when both libraries hold the same kernel
symbols and every unit with kernels has a byte-identical ``.text``.

  python scripts/code_object_diff.py old/libvoxnav.so new/libvoxnav.so
"""
from __future__ import annotations

import hashlib
import json
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
                        "text_sha256": hashlib.sha256(blob).hexdigest()})
    return out


def main(old: Path, new: Path) -> int:
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
    rep["kernel_free_units_new"] = [{"text_bytes": u["text_bytes"], "objects": u["objects"]}
                                    for u in b if not u["kernels"]]
    rep["ok"] = ok
    print(json.dumps(rep, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(Path(sys.argv[1]), Path(sys.argv[2])))

"""The encoder behind vn_import_state (csrc/env_state.h) and the env-state files, on the CPU.

The header is compiled with a stand-alone driver (tests/host/env_import_check.cpp) under g++ with
AddressSanitizer and UBSan and run as a child process, like tests/test_env_plan.py does for the plan.
Every expectation is worked out by hand from the rules of the import (include/voxnav.h,
vn_import_state), not printed from the code under test.
"""
import shutil
import subprocess

import numpy as np
import pytest

from helpers import REPO

CSRC = REPO / "3d-navigation-reinforcement-learning_amd" / "csrc"
DRIVER = REPO / "tests" / "host" / "env_import_check.cpp"
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/env_import_check.cpp"
    exe = tmp_path_factory.mktemp("env_import") / "env_import_check"
    cmd = [cxx, *CXXFLAGS, "-I", str(CSRC), "-I", str(REPO / "include"), str(DRIVER), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(script: str):
        p = subprocess.run([str(exe)], input=script, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, f"driver exit {p.returncode}\n{p.stderr[-4000:]}"
        return p.stdout.splitlines()
    return run


# ------------------------------------------------------------------------------------------- codec
def test_codec_values(driver):
    # (value, wall, latent-wall mode) -> byte: bit7 known, bit6 wall, bits 0-5 the count, saturating at 63
    cases = [((-1, 0, 0), 0x00), ((-1, 1, 0), 0x00), ((-1, 0, 1), 0x00), ((-1, 1, 1), 0x40),
             ((0, 0, 0), 0x80), ((7, 0, 0), 0x87), ((63, 0, 1), 0xBF), ((64, 0, 0), 0xBF), ((200, 0, 0), 0xBF),
             ((-2, 1, 0), 0xC0), ((-2, 1, 1), 0xC0)]
    lines = driver("".join("codec %d %d %d\n" % c for c, _ in cases))
    assert [int(ln.split("=")[1], 16) for ln in lines] == [b for _, b in cases]


def test_decode_is_the_exports_rule(driver):
    # known through the byte or through a plane; bit6 of a known cell = wall; else the count
    cases = [("00", 0, -1), ("40", 0, -1), ("00", 1, 0), ("40", 1, -2), ("80", 0, 0), ("87", 0, 7), ("bf", 1, 63),
             ("c0", 0, -2)]
    lines = driver("".join("decode %s %d\n" % (b, p) for b, p, _ in cases))
    assert [int(ln.split("=")[1]) for ln in lines] == [v for _, _, v in cases]


def test_cell_predicate(driver):
    # inside the room: nothing below -2, -2 only at a wall, a known free value only at a free cell
    cases = [((-1, 0), 1), ((-1, 1), 1), ((-2, 1), 1), ((-2, 0), 0), ((0, 0), 1), ((0, 1), 0), ((5, 1), 0),
             ((127, 0), 1), ((-3, 0), 0), ((-3, 1), 0), ((-128, 1), 0)]
    lines = driver("".join("cell %d %d\n" % c for c, _ in cases))
    assert [int(ln.split("=")[1]) for ln in lines] == [ok for _, ok in cases]


def test_counters_above_their_fields_are_clamped(driver):
    # step_count has 24 bits in the hot state, bump_count 26; both saturate on the device
    lines = driver("clamp 5 7\nclamp %d %d\nclamp %d %d\n" % (2 ** 24 - 1, 2 ** 26 - 1, 2 ** 24 + 5, 2 ** 40))
    assert lines == ["steps=5 bumps=7", "steps=16777215 bumps=67108863", "steps=16777215 bumps=67108863"]


# ------------------------------------------------------------------------------- one agent, by hand
W, D, H, L = 9, 6, 3, 4


def room_walls():
    w = np.ones((W, D, H), bool)
    w[1:-1, 1:-1, 1:-1] = False
    w[4, 3, 1] = True                                                       # one interior wall
    return w


def small_room():
    return np.array([[[1, 1, 1]] * 3, [[1, 1, 1], [1, 0, 1], [1, 1, 1]], [[1, 1, 1]] * 3], bool)   # 3 x 3 x 3 shell


# x, y, z, facing, last_action, step_count, visited, bumps, done, last_bump, near_wall, was_near_wall, cid, room,
# max_steps (ignored), next_seed
STATE = [2, 3, 1, 1, 4, 17, 2, 3, 0, 1, 0, 1, 2, 1, 12345, 4000000000]
# the imported map: the agent's own cell 3, a cell visited 70 times, a known free cell, a known wall
CELLS = [(2, 3, 1, 3), (6, 1, 1, 70), (6, 2, 1, 0), (8, 1, 1, -2)]


def agent_script(cap, state=STATE, cells=CELLS, outside=99, defer=-1):
    rooms = [small_room(), room_walls()]                                    # the agent is in room 1
    out = ["agent %d %d %d %d" % (cap, defer, L, len(rooms))]
    for w in rooms:
        out.append("%d %d %d %s" % (*w.shape, "".join("01"[int(b)] for b in w.ravel())))
    out.append(" ".join(str(v) for v in state))
    out.append("%d %d" % (outside, len(cells)))
    out += ["%d %d %d %d" % c for c in cells]
    return "\n".join(out) + "\n"


def parsed(lines):
    kv = dict(ln.split("=", 1) for ln in lines)
    out = {"verdict": kv["verdict"]}
    if kv["verdict"] == "ok":
        out["layout"] = {k: int(v) for k, v in (t.split(":") for t in kv["layout"].split())}
        out["sense"] = {k: int(v) for k, v in (t.split(":") for t in kv["sense"].split())}
        for k in ("map", "xplane", "yplane"):
            out[k] = {int(a): int(b, 16) for a, b in (t.split(":") for t in kv[k].split())}
        out["nz"] = [int(v, 16) for v in kv["nz"].split()]
        out["stood"] = [int(v, 16) for v in kv["stood"].split()]
        out["window"] = [int(v, 16) for v in kv["window"].split()]
        out["decoded"] = np.array([int(v) for v in kv["decoded"].split()]).reshape(W, D, H)
    return out


def bcol(x, y, nby=2):
    return (((x >> 2) * nby + (y >> 2)) << 4) + ((x & 3) << 2 | (y & 3))


# What get_obs's six rays from (2, 3, 1) see with L = 4 (by hand): +x one free cell then the interior wall,
# -x one free cell then the shell, +y one then the shell, -y two then the shell, the shell directly above and below.
SENSED = {(3, 3, 1): 0x80, (4, 3, 1): 0xC0, (1, 3, 1): 0x80, (0, 3, 1): 0xC0, (2, 4, 1): 0x80, (2, 5, 1): 0xC0,
          (2, 2, 1): 0x80, (2, 1, 1): 0x80, (2, 0, 1): 0xC0, (2, 3, 2): 0xC0, (2, 3, 0): 0xC0}
KNOWN = {**SENSED, (2, 3, 1): 0x83, (6, 1, 1): 0xBF, (6, 2, 1): 0x80, (8, 1, 1): 0xC0}   # 70 saturates at 63
# x-plane row (y, z) = word y * 8 + z holds bit x of every known cell; y-plane row (x, z) = word x * 8 + z bit y
XPLANE = {3 * 8 + 1: 0x1F, 4 * 8 + 1: 0x04, 5 * 8 + 1: 0x04, 2 * 8 + 1: 0x44, 1 * 8 + 1: 0x144, 0 * 8 + 1: 0x04,
          3 * 8 + 2: 0x04, 3 * 8 + 0: 0x04}
YPLANE = {2 * 8 + 1: 0x3F, 2 * 8 + 2: 0x08, 2 * 8 + 0: 0x08, 0 * 8 + 1: 0x08, 1 * 8 + 1: 0x08, 3 * 8 + 1: 0x08,
          4 * 8 + 1: 0x08, 6 * 8 + 1: 0x06, 8 * 8 + 1: 0x02}


def expected_dense():
    d = np.full((W, D, H), -1)
    for (x, y, z), b in KNOWN.items():
        d[x, y, z] = -2 if b == 0xC0 else b & 0x3F
    return d


def test_planes_are_consistent_with_the_hand_made_known_set():
    for (x, y, z) in KNOWN:                                                # the two tables above name the same cells
        assert XPLANE[y * 8 + z] >> x & 1 and YPLANE[x * 8 + z] >> y & 1
    ones = lambda rows: sum(bin(v).count("1") for v in rows.values())   # noqa: E731
    assert ones(XPLANE) == len(KNOWN) == ones(YPLANE)


def test_agent_in_u32_plane_set_mode(driver):
    t = parsed(driver(agent_script(-1)))
    assert t["verdict"] == "ok"
    # 12 x 8 padded columns of 8 bytes in 3 x 2 bricks; 8 * 8 x rows and 12 * 8 y rows of 4 bytes
    assert t["layout"] == dict(pw=12, pd=8, ph=8, nby=2, pcache=2, nwx=1, nwy=1, xp_off=768, yp_off=768 + 256,
                               agent_bytes=768 + 256 + 384)
    assert t["sense"] == dict(near=1, cid=0, move_mask=0xF)                 # walls above and below; four free moves
    assert t["xplane"] == XPLANE and t["yplane"] == YPLANE
    # the byte map: the two columns the agent stood in (they hold a count) in full, with the latent bit at
    # their unknown walls; every other column as the room image, its known cells being in the planes
    walls = room_walls()
    want = {bcol(x, y) * 8 + z: 0x40 for x, y, z in np.argwhere(walls)}
    want.update({bcol(2, 3) * 8 + 0: 0xC0, bcol(2, 3) * 8 + 1: 0x83, bcol(2, 3) * 8 + 2: 0xC0,
                 bcol(6, 1) * 8 + 0: 0x40, bcol(6, 1) * 8 + 1: 0xBF, bcol(6, 1) * 8 + 2: 0x40})
    assert t["map"] == want
    assert t["stood"] == [0, 1 << 6, 0, 1 << 2] + [0] * 28                  # rows y = 1 and y = 3
    assert t["nz"] == [0x3F, 0x15F]                                        # x sets y' = 0..5; y sets x' = 0-4, 6, 8
    np.testing.assert_array_equal(t["decoded"], expected_dense())
    # window value 16 i + 4 q + k is cell (x + i - 2, y + q - 2, z + k - 2) = (i, q + 1, k - 1)
    win = t["window"]
    assert (win[42], win[58], win[43], win[41], win[40]) == (0x83, 0x80, 0xC0, 0xC0, 0x00)
    assert win[2] == 0x40 and win[6] == 0x40                                # (0,1,1), (0,2,1): latent shell walls
    assert win[16 * 1 + 4 * 0 + 2] == 0x00                                  # (1,1,1): free and unknown


def test_window_cell_at_wall_is_latent_only_where_the_room_has_one(driver):
    t = parsed(driver(agent_script(-1)))
    walls = room_walls()
    for o, b in enumerate(t["window"]):
        x, y, z = (o >> 4), ((o >> 2) & 3) + 1, (o & 3) - 1
        if not 0 <= z < H:
            assert b == 0, o                                               # below / above the room
        elif (x, y, z) in KNOWN:
            assert b == KNOWN[(x, y, z)], o
        else:
            assert b == (0x40 if walls[x, y, z] else 0x00), o


@pytest.mark.parametrize("cap,defer,pcache", [(0, -1, 0), (0, 0, 0), (1, -1, 1)])
def test_agent_in_u64_row_modes(driver, cap, defer, pcache):
    t = parsed(driver(agent_script(cap, defer=defer)))
    assert t["verdict"] == "ok"
    assert t["layout"] == dict(pw=12, pd=8, ph=8, nby=2, pcache=pcache, nwx=1, nwy=1, xp_off=768, yp_off=768 + 512,
                               agent_bytes=768 + 512 + 768)
    assert t["xplane"] == XPLANE and t["yplane"] == YPLANE                  # the same bits in 8-byte rows
    if pcache == 0:     # byte marks: every known cell's byte, nothing else (no latent walls)
        assert t["map"] == {bcol(x, y) * 8 + z: b for (x, y, z), b in KNOWN.items()}
    else:               # plane sets: as in u32 mode
        want = {bcol(x, y) * 8 + z: 0x40 for x, y, z in np.argwhere(room_walls())}
        want.update({bcol(2, 3) * 8 + 0: 0xC0, bcol(2, 3) * 8 + 1: 0x83, bcol(2, 3) * 8 + 2: 0xC0,
                     bcol(6, 1) * 8 + 1: 0xBF})
        assert t["map"] == want
    np.testing.assert_array_equal(t["decoded"], expected_dense())


def test_cells_outside_the_room_are_ignored(driver):
    a = parsed(driver(agent_script(-1, outside=99)))
    b = parsed(driver(agent_script(-1, outside=-77)))                       # not even a valid value
    assert a["map"] == b["map"] and a["xplane"] == b["xplane"] and a["yplane"] == b["yplane"]
    np.testing.assert_array_equal(a["decoded"], b["decoded"])


def with_field(i, v):
    s = list(STATE)
    s[i] = v
    return s


REJECTED = [
    ("room below 0", with_field(13, -1), CELLS, "scalars"),
    ("room past the set", with_field(13, 2), CELLS, "scalars"),
    ("x at W", with_field(0, W), CELLS, "position"),
    ("y below 0", with_field(1, -1), CELLS, "position"),
    ("z at H", with_field(2, H), CELLS, "position"),
    ("huge x", with_field(0, 2 ** 40), CELLS, "position"),
    ("on the interior wall", with_field(0, 4), CELLS, "wall"),
    ("on the shell", with_field(2, 0), CELLS, "wall"),
    ("facing 4", with_field(3, 4), CELLS, "scalars"),
    ("facing -1", with_field(3, -1), CELLS, "scalars"),
    ("last_action 6", with_field(4, 6), CELLS, "scalars"),
    ("done 2", with_field(8, 2), CELLS, "scalars"),
    ("last_bump -1", with_field(9, -1), CELLS, "scalars"),
    ("near_wall 2", with_field(10, 2), CELLS, "scalars"),
    ("was_near_wall 3", with_field(11, 3), CELLS, "scalars"),
    ("cells_insight_down L + 1", with_field(12, L + 1), CELLS, "scalars"),
    ("cells_insight_down -1", with_field(12, -1), CELLS, "scalars"),
    ("seed 2^32", with_field(15, 2 ** 32), CELLS, "scalars"),
    ("seed -1", with_field(15, -1), CELLS, "scalars"),
    ("step_count -1", with_field(5, -1), CELLS, "scalars"),
    ("visited -1", with_field(6, -1), CELLS, "scalars"),
    ("bump_count -1", with_field(7, -1), CELLS, "scalars"),
    ("visited above the room's cells", with_field(6, W * D * H + 1), CELLS, "position"),
    ("0 at a wall", STATE, CELLS + [(0, 0, 0, 0)], "cells"),
    ("a count at the interior wall", STATE, CELLS + [(4, 3, 1, 2)], "cells"),
    ("-2 at a free cell", STATE, CELLS + [(5, 2, 1, -2)], "cells"),
    ("-3", STATE, CELLS + [(5, 2, 1, -3)], "cells"),
    ("own cell unknown", STATE, [(2, 3, 1, -1)] + CELLS[1:], "cells"),
    ("own cell 0", STATE, [(2, 3, 1, 0)] + CELLS[1:], "cells"),
]


@pytest.mark.parametrize("name,state,cells,verdict", REJECTED, ids=[r[0] for r in REJECTED])
def test_each_rejection_rule(driver, name, state, cells, verdict):
    for cap in (-1, 0):
        assert parsed(driver(agent_script(cap, state=state, cells=cells)))["verdict"] == verdict


def test_limits_that_are_accepted(driver):
    # the largest seed, cells_insight_down = L, max_steps (field 14) anything, counters past their fields (clamped)
    s = list(STATE)
    s[15], s[12], s[14], s[5], s[7] = 2 ** 32 - 1, L, -999, 2 ** 30, 2 ** 30
    assert parsed(driver(agent_script(-1, state=s)))["verdict"] == "ok"


# ------------------------------------------------------------------------------------ env-state files
class FakeEnv:
    """What save_env_state / load_env_state use of an env, on CPU tensors."""

    def __init__(self, variant=0):
        import torch
        self.variant, self._t, self.torch = variant, 137, torch
        g = torch.Generator().manual_seed(3)
        self.state = torch.randint(0, 50, (5, 16), generator=g, dtype=torch.int64)
        self.map = torch.randint(-2, 60, (5, 8, 8, 8), generator=g, dtype=torch.int64).to(torch.int8)
        self.blob = torch.randint(0, 256, (1000,), generator=g, dtype=torch.int64).to(torch.uint8)
        self.tag = 0xFEDCBA9876543210                                      # needs all 64 bits
        self.imported = self.restored = None

    def export_state(self):
        return self.state

    def belief(self):
        return self.map

    def snapshot(self):
        from voxnav.env import EnvSnapshot
        return EnvSnapshot(self.tag, self.blob, self._t)

    def import_state(self, state, belief):
        self.imported = (state, belief)

    def restore(self, snap):
        self.restored = snap
        self._t = snap.t


def test_portable_file_round_trip(tmp_path):
    from voxnav.checkpoint import load_env_state, save_env_state
    src, dst = FakeEnv(), FakeEnv()
    dst._t = 0
    path = save_env_state(tmp_path / "env", src)
    assert path.suffix == ".npz"
    with np.load(path) as z:
        assert str(z["form"]) == "portable" and int(z["format_version"]) == 1 and int(z["t"]) == 137
    load_env_state(path, dst)
    st, bl = dst.imported
    assert st.dtype == src.torch.int64 and bl.dtype == src.torch.int8
    assert src.torch.equal(st, src.state) and src.torch.equal(bl, src.map) and dst._t == 137 and dst.restored is None


def test_raw_file_round_trip(tmp_path):
    from voxnav.checkpoint import load_env_state, save_env_state
    for variant, raw in ((1, None), (0, True)):                             # simpleEnv: raw by default
        src, dst = FakeEnv(variant), FakeEnv(variant)
        dst._t = 0
        path = save_env_state(tmp_path / f"env{variant}.npz", src, raw=raw)
        with np.load(path) as z:
            assert str(z["form"]) == "raw" and sorted(z.files) == ["blob", "form", "format_version", "t", "tag"]
        load_env_state(path, dst)
        snap = dst.restored
        assert snap.tag == src.tag and snap.t == 137 and dst._t == 137 and dst.imported is None
        assert snap.data.dtype == src.torch.uint8 and src.torch.equal(snap.data, src.blob)
    with pytest.raises(ValueError, match="CubicEnv variant only"):
        save_env_state(tmp_path / "no.npz", FakeEnv(1), raw=False)


def test_unknown_format_version_is_refused(tmp_path):
    from voxnav.checkpoint import load_env_state, save_env_state
    path = save_env_state(tmp_path / "env.npz", FakeEnv())
    with np.load(path) as z:
        fields = {k: z[k] for k in z.files}
    fields["format_version"] = np.int64(2)
    np.savez(tmp_path / "v2.npz", **fields)
    dst = FakeEnv()
    with pytest.raises(ValueError, match="format version 2"):
        load_env_state(tmp_path / "v2.npz", dst)
    del fields["format_version"]
    np.savez(tmp_path / "v0.npz", **fields)
    with pytest.raises(ValueError, match="format version None"):
        load_env_state(tmp_path / "v0.npz", dst)
    assert dst.imported is None and dst.restored is None

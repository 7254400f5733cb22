"""CPU-side checks of how the engine's sources are cut: every unit is one the build hashes and
links, the HPKE / request units see no Prio3 kernel, the HPKE host unit sees no kernel at all, and
every HPKE kernel header belongs to one unit."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "janus_amd" / "csrc"
HPKE_UNITS = sorted(p.name for p in CSRC.glob("engine_hpke*.hip"))


def _reached(name):
    """(includer, include) for `name`'s own includes and those of the csrc headers they name."""
    seen, todo, edges = set(), [name], []
    while todo:
        cur = todo.pop()
        text = (CSRC / cur).read_text()
        for inc in re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', text, re.M):
            edges.append((cur, inc))
            if inc not in seen and (CSRC / inc).is_file():
                seen.add(inc)
                todo.append(inc)
    return seen, edges


def test_every_unit_is_built():
    from janus_amd._lib import SOURCES
    units = sorted(p.name for p in CSRC.iterdir() if p.suffix in (".hip", ".cpp"))
    assert units == sorted(SOURCES)


def test_per_lane_hpke_headers_are_free_of_hip():
    """What a lane of the HPKE kernels computes lives in headers a plain C++ compiler builds (the
    CPU tests run them); the kernels stay in hpke_dh_gpu.h, hpke_gpu.h, helper_request.h and
    hpke_seal_gpu.h."""
    for name in ("x25519.h", "hpke_kdf256.h", "aes_gcm.h", "hpke_lane.h"):
        text = (CSRC / name).read_text()
        assert "hip_runtime" not in text and "__global__" not in text, name


def test_hpke_unit_includes_no_prio3_kernel_header():
    """The HPKE units reach the Prio3 side through the public prio3gpu_helper_init alone; the
    header they share with engine.hip carries no kernel either."""
    banned = re.compile(r"prio3_kernels\.h|fpvec_\w*\.h|wires_mfma\.h")
    assert "engine_hpke.hip" in HPKE_UNITS and len(HPKE_UNITS) > 1
    for name in HPKE_UNITS + ["engine_internal.h"]:
        seen, edges = _reached(name)
        for _, inc in edges:
            assert not banned.search(inc), (name, inc)
        assert seen, name


def test_hpke_host_unit_reaches_no_kernel():
    """engine_hpke.hip is the host side alone: neither it nor the launch header it calls the
    kernel units through reaches a header that defines a kernel."""
    for name in ("engine_hpke.hip", "hpke_launch.h"):
        assert "__global__" not in (CSRC / name).read_text(), name
        seen, _ = _reached(name)
        assert "hpke_launch.h" in seen | {name}
        for inc in sorted(seen):
            assert "__global__" not in (CSRC / inc).read_text(), (name, inc)


def test_every_hpke_kernel_header_belongs_to_one_unit():
    """A header with an HPKE kernel is reached by exactly one unit, so its kernels are compiled
    (and a change to them recompiled) once; the units together reach at least the kernel headers
    the launch header's families come from."""
    owners = {}
    for unit in sorted(p.name for p in CSRC.glob("*.hip")):
        for inc in _reached(unit)[0]:
            if "__global__" in (CSRC / inc).read_text():
                owners.setdefault(inc, []).append(unit)
    hpke = {h: u for h, u in owners.items() if any(x in HPKE_UNITS for x in u)}
    assert {"hpke_dh_gpu.h", "hpke_gpu.h", "helper_request.h", "hpke_seal_gpu.h",
            "hpke_open_team.h", "hpke_seal_team.h", "hpke_team_split.h"} <= set(hpke)
    for header, units in sorted(hpke.items()):
        assert len(units) == 1, (header, units)

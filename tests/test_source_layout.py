"""CPU-side checks of how the engine's sources are cut: every unit is one the build hashes and
links, and the HPKE / request unit sees no Prio3 kernel."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "janus_amd" / "csrc"


def test_every_unit_is_built():
    from janus_amd._lib import SOURCES
    units = sorted(p.name for p in CSRC.iterdir() if p.suffix in (".hip", ".cpp"))
    assert units == sorted(SOURCES)


def test_per_lane_hpke_headers_are_free_of_hip():
    """What a lane of the HPKE kernels computes lives in headers a plain C++ compiler builds (the
    CPU tests run them); the kernels stay in hpke_gpu.h, helper_request.h and hpke_seal_gpu.h."""
    for name in ("x25519.h", "hpke_kdf256.h", "aes_gcm.h", "hpke_lane.h"):
        text = (CSRC / name).read_text()
        assert "hip_runtime" not in text and "__global__" not in text, name


def test_hpke_unit_includes_no_prio3_kernel_header():
    """engine_hpke.hip reaches the Prio3 side through the public prio3gpu_helper_init alone; the
    header it shares with engine.hip carries no kernel either."""
    banned = re.compile(r"prio3_kernels\.h|fpvec_\w*\.h|wires_mfma\.h")
    for name in ("engine_hpke.hip", "engine_internal.h"):
        seen, todo = set(), [name]
        while todo:  # the unit's own includes and those of the csrc headers they name
            text = (CSRC / todo.pop()).read_text()
            for inc in re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', text, re.M):
                assert not banned.search(inc), (name, inc)
                if inc not in seen and (CSRC / inc).is_file():
                    seen.add(inc)
                    todo.append(inc)
        assert seen, name

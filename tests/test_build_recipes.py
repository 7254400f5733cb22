"""Every recipe that builds the engine library names the units janus_amd/_lib.py builds: the Rust
build script and the A/B variant script compile and link all of SOURCES (a unit left out leaves
the library with undefined symbols, which the build hash cannot show), and the resource-remark
tool compiles every HIP unit."""
import re
from pathlib import Path

from janus_amd._lib import SOURCES

ROOT = Path(__file__).resolve().parent.parent
UNIT = re.compile(r"[\w]+\.(?:hip|cpp)\b")


def _units(path):
    return set(UNIT.findall((ROOT / path).read_text()))


def test_rust_build_script_compiles_every_unit():
    assert _units("rust/aggregator/build.rs") == set(SOURCES)


def test_variant_script_compiles_every_unit():
    assert _units("tools/build_variant.sh") == set(SOURCES)


def test_resource_remark_tool_compiles_every_hip_unit():
    assert _units("tools/kres.sh") == {s for s in SOURCES if s.endswith(".hip")}

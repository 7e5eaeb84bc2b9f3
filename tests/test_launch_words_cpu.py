"""The control words of a scatter launch and of a track launch are a data format shared by the kernels and the host:
their layout is defined once (``ScatterWord`` and ``TrackWord`` in ``csrc/common.hpp``) and every reader and writer
uses the names.  A source check: a renumbered word must not compile cleanly against a bare number somewhere else."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "attpc_engine_amd" / "csrc"
SOURCES = sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.hpp")))


def _enumerators(text: str, enum: str) -> list[str]:
    body = re.search(rf"enum {enum}\b[^{{]*\{{(.*?)\}};", text, re.S)
    assert body, f"enum {enum} not found in common.hpp"
    lines = [line.split("//")[0] for line in body.group(1).splitlines() if not line.strip().startswith("#")]
    return sorted(set(re.findall(r"\b([A-Z][A-Z0-9_]*)\s*=", "\n".join(lines))))


def test_no_control_word_is_addressed_by_a_bare_number():
    assert len(SOURCES) > 10
    indexed = re.compile(r"\w*ctrl\w*\s*\[\s*\d")                      # h_ctrl[2], a.out.ctrl[8 + k], ctrl[8] = {...}
    offset = re.compile(r"\w*ctrl\w*(\.p)?\s*\)?\s*\+\s*\d")           # static_cast<uint32_t*>(ts.ctrl.p) + 3
    hits = [f"{src.name}:{n}: {line.strip()}" for src in SOURCES for n, line in enumerate(src.read_text().splitlines(), 1)
            if indexed.search(line) or offset.search(line)]
    assert not hits, "\n".join(hits)


def test_every_control_word_is_defined_in_one_place():
    common = (CSRC / "common.hpp").read_text()
    scatter, track = _enumerators(common, "ScatterWord"), _enumerators(common, "TrackWord")
    for wanted in ("CTRL_ROW_CURSOR", "CTRL_SEG_CURSOR", "CTRL_OVERFLOW", "CTRL_NEXT_EVENT", "CTRL_LONE", "CTRL_ROWS", "CTRL_DANGER", "CTRL_WORDS"):
        assert wanted in scatter, scatter
    for wanted in ("TRK_NEXT_TRACK", "TRK_NEXT_BLOCK", "TRK_OVERFLOW", "TRK_AT_LIMIT", "TRK_CAPPED", "TRK_WORDS"):
        assert wanted in track, track
    for name in scatter + track:
        defined_in = [src.name for src in SOURCES if re.search(rf"\b{name}\s*=(?!=)", src.read_text())]
        assert defined_in == ["common.hpp"], (name, defined_in)
        used_in = [src.name for src in SOURCES if src.name != "common.hpp" and re.search(rf"\b{name}\b", src.read_text())]
        assert used_in, f"{name} is never used"


def test_the_host_file_holds_no_kernel_and_no_launch():
    text = (CSRC / "abi.hip").read_text()
    assert "__global__" not in text
    assert "hipLaunchKernelGGL" not in text

"""The size limit of the pad look-up table (attpc_det_configure, csrc/abi.hip) against what the scatter kernel's gather
addressing rests on (csrc/scatter.hip, lut_offsets()): an index <= lut_n times the byte pitch 2 (lut_n + 1), as two
16-bit factors of v_mad_u32_u16.  No device needed: the limit is read from the source, where the refusal is one line."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "attpc_engine_amd" / "csrc"


def test_lookup_table_limit_keeps_both_offset_factors_16_bit():
    text = (CSRC / "abi.hip").read_text()
    limits = [int(v) for v in re.findall(r"d->lut_n > (\d+)\) return fail\(ctx, ATTPC_E_INVALID", text)]
    assert len(limits) == 1, limits  # one refusal, ahead of everything that reads the table
    limit = limits[0]
    assert limit == 32000
    assert limit < 2 ** 15 and 2 * (limit + 1) < 2 ** 16  # the largest index (lut_n itself) and the byte pitch
    assert limit * 2 * (limit + 1) + 2 * limit < 2 ** 32  # the largest byte offset of a gather
    assert "v_mad_u32_u16" in (CSRC / "scatter.hip").read_text()  # (the reason for the bound is still there)

"""CPU sanitizer builds of the host-only packed-trace code (csrc/trace_pack_host.cpp: attpc_trace_pack_host,
attpc_trace_unpack and the decoder's thread pool) under ASan + UBSan and under ThreadSanitizer, driven by the
stand-alone program tests/native/trace_pack_san.cpp -- no Python in the process, no GPU."""
import os
import subprocess
from pathlib import Path

import pytest

from tests.test_native_sanitizers import _gxx, _without_aslr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "attpc_engine_amd" / "csrc"


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name,flags", [
    ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
    ("tsan", ["-fsanitize=thread"]),
])
def test_trace_pack_host_under_sanitizers(tmp_path, name, flags):
    """The round trip of 40 000 mixed rows through exactly-sized heap arrays with 1 ... 16 decoder threads, a run of
    rows decoded alone, and every malformed record of the contract refused: no out-of-bounds access, no undefined
    behaviour, no data race; every sample checked."""
    exe = tmp_path / f"trace_pack_{name}"
    cmd = [_gxx(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", f"-I{CSRC}", *flags,
           str(ROOT / "tests" / "native" / "trace_pack_san.cpp"), str(CSRC / "trace_pack_host.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run(_without_aslr([str(exe)]) if name == "tsan" else [str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "mismatches 0 unexpected 0" in run.stdout
    assert "ERROR" not in run.stderr and "WARNING: ThreadSanitizer" not in run.stderr, run.stderr[-4000:]

"""Kernel-by-kernel comparison of the gfx950 code of two library builds (no GPU needed):
    python tools/compare_isa.py before.so after.so [old=new ...]
Per kernel: are the instruction texts (addresses stripped) identical, or at least the mnemonic sequences, and the
resources of the code-object notes (VGPRs, SGPRs, LDS bytes, private_segment_fixed_size); for every kernel, whether each
barrier waits for the wave's LDS operations (tests/isa_tools.py).  Kernels are matched by name without namespace and
argument list; ``old=new`` (e.g. ``'estimate_kernel=estimate_kernel<0>'``) compares the kernel ``old`` of before.so with
``new`` of after.so, for a kernel that became an instantiation of a template.  Prints a markdown table."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.isa_tools import barriers_without_lds_wait, device_code_objects, disassemble_objects, llvm_tool  # noqa: E402

FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels_of(library: Path) -> dict:
    """{kernel symbol: (instructions, {note field: value})}"""
    with tempfile.TemporaryDirectory() as tmp:
        objects = device_code_objects(library, Path(tmp))
        functions = disassemble_objects(objects)
        notes = {}
        for co in objects:
            text = subprocess.run([str(llvm_tool("llvm-readelf")), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
            for block in text.split("\n  - .agpr_count:")[1:]:
                name = re.search(r"^\s*\.name:\s*(\S+)", block, re.M).group(1)
                notes[name] = {f: int(re.search(rf"^\s*\{f}:\s*(\d+)", block, re.M).group(1)) for f in FIELDS}
    return {short_name(name): (functions[name], notes[name]) for name in notes}


def short_name(symbol: str) -> str:
    """`sc_big::scatter_kernel<0,1>` for `_ZN5attpc6sc_big14scatter_kernelILb0ELb1EEEvNS_11ScatterArgsE`: a kernel keeps
    this name when it moves to another file or namespace, or when its argument list changes."""
    parts, rest = [], symbol[3:] if symbol.startswith("_ZN") else symbol
    while (m := re.match(r"(\d+)", rest)):
        n = int(m.group(1))
        parts.append(rest[m.end(): m.end() + n])
        rest = rest[m.end() + n:]
        if parts[-1].endswith("_kernel"):
            break
    bools = re.match(r"I((?:Lb\dE)+)E", rest)
    name = "::".join(part for part in parts if part != "attpc" and not part.startswith("_GLOBAL__N"))
    return name + ("<" + ",".join(re.findall(r"Lb(\d)E", bools.group(1))) + ">" if bools else "")


def text_of(insns: list) -> list:
    """Instruction texts without the padding behind the kernel's end (it depends on what follows in the code object)."""
    text = [t for _, t in insns]
    while text and text[-1].split()[0] in ("s_nop", "s_code_end"):
        text.pop()
    return text


def main() -> None:
    before, after = kernels_of(Path(sys.argv[1])), kernels_of(Path(sys.argv[2]))
    for old, new in (arg.split("=", 1) for arg in sys.argv[3:]):
        before[new] = before.pop(old)
    print("| kernel | text | mnemonics | instructions | VGPR | SGPR | LDS | scratch | bare barriers |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in sorted(set(before) | set(after)):
        if name not in before or name not in after:
            print(f"| `{name}` | only in {'after' if name in after else 'before'} | | | | | | | |")
            continue
        (ia, na), (ib, nb) = before[name], after[name]
        ta, tb = text_of(ia), text_of(ib)
        ma, mb = [t.split()[0] for t in ta if t], [t.split()[0] for t in tb if t]
        res = [f"{na[f]}" if na[f] == nb[f] else f"{na[f]} -> {nb[f]}" for f in FIELDS]
        count = f"{len(ta)}" if len(ta) == len(tb) else f"{len(ta)} -> {len(tb)}"
        print(f"| `{name}` | {'same' if ta == tb else 'DIFFERS'} | {'same' if ma == mb else 'DIFFERS'} | {count} | "
              + " | ".join(res) + f" | {len(barriers_without_lds_wait(ib))} |")


if __name__ == "__main__":
    main()

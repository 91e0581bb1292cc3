#!/usr/bin/env python3
"""One line per kernel of a device code object, for comparing two builds of the same source:

    hipcc <flags> --offload-device-only --no-gpu-bundle-output -c -o new.co source.hip
    tools/kernel_digest.py new.co > new.txt          # ... the same for the other build, then diff

Each line: the kernel's symbol, its vgpr_count, sgpr_count, group_segment_fixed_size and private_segment_fixed_size
from the code object's metadata note (llvm-readelf --notes), and the SHA-256 of its disassembly (llvm-objdump -d)
with the addresses stripped (each line's own, and the pc-relative displacement of a global behind s_getpc_b64, which
moves when any other kernel of the object grows, shrinks, comes or goes).  Sorted by symbol.  A digest only: it looks for nothing and judges nothing.
"""
import hashlib
import os
import re
import subprocess
import sys

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def kernel_notes(path):
    """{symbol without .kd: {field: value}} from the amdhsa.kernels list of the metadata note"""
    kernels, current, inside = [], None, False
    for line in run("llvm-readelf", "--notes", path).splitlines():
        if not line.startswith(" "):  # a top-level key of the note
            inside = line.startswith("amdhsa.kernels:")
            continue
        # a kernel's own fields are indented by four columns ("  - .first:" opens the kernel); .args' are deeper
        m = re.match(r"^  (- |  )\.(\w+):\s*(.*)$", line) if inside else None
        if not m:
            continue
        if m.group(1) == "- ":
            current = {}
            kernels.append(current)
        current[m.group(2)] = m.group(3).strip().strip("'\"")
    return {k["symbol"][:-3]: {f: k.get(f, "?") for f in FIELDS} for k in kernels if k.get("symbol", "").endswith(".kd")}


def disassembly(path):
    """{symbol: [instruction lines without their addresses]}"""
    text, symbol, after_getpc = {}, None, 0
    for line in run("llvm-objdump", "-d", path).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            symbol = m.group(1)
            text[symbol] = []
        elif symbol is not None and line.strip() == "...":
            continue  # zero padding up to the next symbol's alignment: it comes and goes with the kernel's neighbours
        elif symbol is not None and line.startswith("\t"):
            # "\tinstruction operands   // 0000000012A4: ENCODING ..." -> without the address
            line = re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line).rstrip()
            # ... and without the displacement that the two adds behind s_getpc_b64 turn the pc into a global's
            # address with: an address too, it moves with the layout of the whole object
            if after_getpc and re.match(r"\ts_addc?_u32 ", line):
                line = re.sub(r", [^,]+//.*$", ", <pc-relative>", line)
            after_getpc = 2 if line.startswith("\ts_getpc_b64") else max(after_getpc - 1, 0)
            text[symbol].append(line)
    return text


def digest(path):
    notes, text = kernel_notes(path), disassembly(path)
    lines = []
    for symbol in sorted(notes):
        sha = hashlib.sha256("\n".join(text.get(symbol, [])).encode()).hexdigest()
        lines.append(" ".join([symbol, *(f"{f}={notes[symbol][f]}" for f in FIELDS), f"sha256={sha}"]))
    return lines


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    print("\n".join(digest(sys.argv[1])))

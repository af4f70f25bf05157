"""Hashes of the device code of translation units, kernel by kernel, with the names left out: two checkouts have the same kernels when
the sorted hashes of a unit are equal (a template pack added to a kernel changes its mangled name and nothing else). Built objects are
read from qgtc_ppopp22_amd/build/ (run build() first); gfx950 code objects are unbundled with the ROCm LLVM tools.

    python tools/kernel_bodies.py qgtc_tiled_float qgtc_tiled_max ... > bodies.txt     # in each checkout, then diff the two files

TILED_UNITS lists the float, extremum and attention units of the tiled adjacency (the families whose shared templates a new trailing
pack element touches), EDGE_UNITS the edge-value units and BIT_UNITS the four units of the quantised products; ATTN_HEADS_UNITS the six units of the attention path with heads; the word
`tiled` / `edge` / `bit` / `attn_heads` on the command line stands for the list.

With --names every line is `unit hash name`, sorted by the kernel's mangled name: two checkouts whose outputs are equal instantiate the
same kernels in every unit, under the same names, with the same instructions (a refactor of the host side must leave it so).

A hash covers the disassembler's text of a kernel, and that text ends in a line `...` where zero bytes pad the kernel to the next one's
256-byte boundary: the last kernel of a code object has no such line. With --code those lines and empty ones are left out, so a kernel
that gains or loses a successor in its unit keeps its hash (compare two checkouts with the same setting).
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILED_UNITS = ("qgtc_tiled_float", "qgtc_tiled_float_t", "qgtc_tiled_float_src", "qgtc_tiled_float_t_src", "qgtc_tiled_float_drop",
               "qgtc_tiled_float_t_drop", "qgtc_tiled_float_nodes", "qgtc_tiled_float_t_nodes", "qgtc_tiled_max", "qgtc_tiled_max_t",
               "qgtc_tiled_max_drop", "qgtc_tiled_max_nodes", "qgtc_tiled_attn", "qgtc_tiled_attn_t", "qgtc_tiled_attn_drop",
               "qgtc_tiled_attn_t_drop", "qgtc_tiled_attn_nodes", "qgtc_tiled_attn_t_nodes")   # 263 kernels
EDGE_UNITS = ("qgtc_tiled_float_edge", "qgtc_tiled_float_t_edge", "qgtc_tiled_sddmm")
BIT_UNITS = ("qgtc_tiled", "qgtc_tiled_t", "qgtc_tiled_scaled", "qgtc_tiled_t_scaled")
ATTN_HEADS_UNITS = ("qgtc_tiled_attn_heads", "qgtc_tiled_attn_heads_t", "qgtc_tiled_attn_heads_drop", "qgtc_tiled_attn_heads_t_drop",
                    "qgtc_tiled_attn_heads_nodes", "qgtc_tiled_attn_heads_t_nodes")
WORDS = {"tiled": TILED_UNITS, "edge": EDGE_UNITS, "bit": BIT_UNITS, "attn_heads": ATTN_HEADS_UNITS}
LLVM = "/opt/rocm/llvm/bin"


def named_bodies(unit, code_only=False):
    """[(mangled name, hash of the body)] of the unit's kernels, in the code object's order"""
    obj = os.path.join(ROOT, "qgtc_ppopp22_amd", "build", unit + ".hip.o")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={fat}", f"--output={co}"], check=True)
        text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True,
                              check=True).stdout
    out, cur, name = [], [], None
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            if name:
                out.append((name, hashlib.md5("\n".join(cur).encode()).hexdigest()))
            name, cur = m.group(1), []
        elif name and not (code_only and line.strip() in ("...", "")):
            cur.append(re.sub(r"//.*$", "", re.sub(r"<[^>]*>", "", line)).strip())
    if name:
        out.append((name, hashlib.md5("\n".join(cur).encode()).hexdigest()))
    return out


def bodies(unit, code_only=False):
    return sorted(h for _, h in named_bodies(unit, code_only))


if __name__ == "__main__":
    names, code = "--names" in sys.argv[1:], "--code" in sys.argv[1:]
    units = []
    for a in sys.argv[1:]:
        units += [] if a in ("--names", "--code") else list(WORDS.get(a, (a,)))
    for unit in units:
        if names:
            for name, h in sorted(named_bodies(unit, code)):
                print(unit, h, name)
        else:
            for h in bodies(unit, code):
                print(unit, h)

"""Per kernel: resource lines and a hash of the instruction stream, to show that a change (a kernel moved to another file, a
compiled-out switch removed) left the device code alone.  Two kernels are the same code when their lines here are equal.

    hipcc <the Makefile's flags> --cuda-device-only -S x.hip -o x.s
    hipcc <the Makefile's flags> --cuda-device-only --no-gpu-bundle-output -c x.hip -o x.o && llvm-objdump -d x.o > x.dis
    python tools/dev/kernel_isa.py x.s x.dis ...

x.s: the compiler's resource lines and its text, with comments, directives and blank lines dropped and the block labels' function
index (.LBB<n>_, the kernel's position in its file) normalised.  Inline asm stands there as written, macros and assembler
conditionals unexpanded: for kernels built from it the disassembly (any other file name) is the stream that counts — the machine
instructions without addresses, encodings and the padding behind the last one."""
import hashlib
import re
import sys

RESOURCES = ("NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy", ".amdhsa_group_segment_fixed_size", ".amdhsa_accum_offset")


def kernels(lines, asm):
    """{symbol: (stream, {resource: value})}"""
    out, cur = {}, None
    for ln in lines:
        head = re.match(r"(\w+):\s*; @\1" if asm else r"[0-9a-f]+ <(\w+)>:", ln)
        code = ln.split(";" if asm else "//", 1)[0].strip()
        if head:
            cur = out[head.group(1)] = ([], {})
            body = True
        elif cur and asm and (m := re.match(r"[;\s]*([.\w]+):?\s+(\S+)", ln)) and m.group(1) in RESOURCES:
            cur[1][m.group(1)] = m.group(2)
        elif cur and asm and re.match(r"\.Lfunc_end\d+:", ln):
            body = False
        elif cur and body and code and code != "..." and (not asm or not code.startswith(".") or code.endswith(":")):
            cur[0].append(re.sub(r"\.LBB\d+_", ".LBB_", code))
    for stream, _ in out.values():
        while not asm and stream and stream[-1].startswith(("s_nop", "s_code_end")):
            stream.pop()
    return {k: v for k, v in out.items() if asm and ".amdhsa_accum_offset" in v[1] or not asm and v[0]}


for path in sys.argv[1:]:
    print(path)
    for name, (stream, res) in sorted(kernels(open(path).read().splitlines(), path.endswith(".s")).items()):
        digest = hashlib.sha256("\n".join(stream).encode()).hexdigest()[:16]
        print(f"  {name}: {len(stream)} lines, sha256 {digest}" + "".join(f" {k}={v}" for k, v in res.items()))

#!/usr/bin/env python3
"""kernel_diff.py A.so B.so — are the gfx950 kernels of two builds of the library the same machine code?

Extracts the gfx950 code objects both libraries embed (llvm-objdump --offloading, as tests/test_abi.py does), disassembles them and
compares symbol by symbol: symbols only one side has, and instruction sequences that differ.  Two things are masked before the
comparison, because they say where a kernel lies in its code object and not what it does:
  * the literals of a pc-relative address pair (s_getpc_b64 sN:M, then s_add_u32 sN, sN, <literal> / s_addc_u32 sM, sM, <literal>);
  * the padding after a kernel's end (s_code_end / s_nop behind the last instruction).
Prints one line per difference and a summary; exit status 1 if anything differs.  Used to hold a change of form (moving kernels
between translation units, say) to "same machine code"."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
PADDING = re.compile(r"^(s_code_end|s_nop\b)")
GETPC = re.compile(r"^s_getpc_b64 s\[(\d+):(\d+)\]")
PAIR_WINDOW = 8          # the two additions follow their s_getpc_b64 within a few instructions


def disassemble(lib_path):
    """{symbol: [instruction sequence, one per code object that defines the symbol]} of the library's gfx950 code objects"""
    funcs = {}
    with tempfile.TemporaryDirectory() as tmp:
        work = os.path.join(tmp, "lib.so")
        shutil.copy(lib_path, work)
        subprocess.check_call([OBJDUMP, "--offloading", work], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
        bundles = sorted(glob.glob(work + ".*gfx950"))
        if not bundles:
            sys.exit(f"{lib_path}: no gfx950 code object")
        for bundle in bundles:
            text = subprocess.check_output([OBJDUMP, "-d", "--mcpu=gfx950", "--no-show-raw-insn", bundle], text=True, stderr=subprocess.DEVNULL)
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = []
                    funcs.setdefault(m.group(1), []).append(cur)
                elif cur is not None and re.match(r"^\s+[a-z_0-9]+", line):
                    ins = line.split("//")[0].strip()
                    if ins:
                        cur.append(ins)
    return funcs


def masked(seq):
    """the sequence without its trailing padding and with the literals of pc-relative pairs replaced by <pcrel>"""
    seq = list(seq)
    while seq and PADDING.match(seq[-1]):
        seq.pop()
    for i, ins in enumerate(seq):
        m = GETPC.match(ins)
        if not m:
            continue
        wanted = {f"s_add_u32 s{m.group(1)}, s{m.group(1)}, ", f"s_addc_u32 s{m.group(2)}, s{m.group(2)}, "}
        for j in range(i + 1, min(i + 1 + PAIR_WINDOW, len(seq))):
            for head in list(wanted):
                if seq[j].startswith(head) and re.fullmatch(r"(0x[0-9a-f]+|-?\d+)", seq[j][len(head):]):
                    seq[j] = head + "<pcrel>"
                    wanted.discard(head)
            if not wanted:
                break
    return seq


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = (disassemble(p) for p in sys.argv[1:3])
    differences = instructions = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"only in {sys.argv[2] if name not in a else sys.argv[1]}: {name}")
            differences += 1
            continue
        sa, sb = sorted(masked(s) for s in a[name]), sorted(masked(s) for s in b[name])
        instructions += sum(len(s) for s in sa)
        if len(sa) != len(sb):
            print(f"defined {len(sa)} / {len(sb)} times: {name}")
            differences += 1
            continue
        for x, y in zip(sa, sb):
            if x != y:
                at = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                print(f"differs: {name}: {len(x)} / {len(y)} instructions, first at {at}: "
                      f"{x[at] if at < len(x) else '<end>'}  |  {y[at] if at < len(y) else '<end>'}")
                differences += 1
    common = sum(1 for n in a if n in b)        # every function symbol of the code objects: kernels, and device functions that were not inlined
    print(f"{common} common symbols, {instructions} instructions compared, " + ("identical" if differences == 0 else f"{differences} differences"))
    return 1 if differences else 0


if __name__ == "__main__":
    sys.exit(main())

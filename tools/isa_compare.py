"""Compare the gfx950 device code of two builds of the library, kernel by
kernel: the set of kernel symbols, each kernel's resource row (the fields of
isa_resources.py) and each kernel's disassembly.  Addresses are taken relative
to the kernel's start, as in isa_dump.py, and the literal of the s_add_u32 /
s_addc_u32 pair that follows an s_getpc_b64 is masked: a PC-relative address
moves with the kernel's place in its code object, not with its code.  The
s_nop padding after a kernel's last instruction is dropped.  Prints
every difference and a summary line; exits 1 if there is any.

    python tools/isa_compare.py OLD.so NEW.so [--rename REGEX=REPLACEMENT]

--rename rewrites OLD's kernel symbols before they are matched, for a change
that adds a defaulted template parameter to a kernel and so renames every
instance without touching its code: k_service's kSolo is
    --rename '(_ZN2pg9k_serviceI\w+?)EEvNS_=\1Lb0EEEvNS_'
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_resources as R  # noqa: E402


def disassembly(co_bytes):
    """{symbol: [line]} of one code object, normalised as described above."""
    with tempfile.NamedTemporaryFile(suffix=".elf") as fh:
        fh.write(co_bytes)
        fh.flush()
        dis = subprocess.run([f"{R.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", fh.name], check=True,
                             capture_output=True, text=True).stdout
    out, cur, base, pc = {}, None, 0, 0
    for line in dis.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", line)
        if m:
            base, cur = int(m.group(1), 16), out.setdefault(m.group(2), [])
            continue
        m = re.match(r"^\s*(.*?)\s*// ([0-9A-F]+):[^<]*(?:<[^+>]*\+(0x[0-9a-f]+)>)?", line)
        if cur is None or not m:
            continue
        insn = m.group(1)
        if insn.startswith("s_getpc_b64"):
            pc = 2  # the next s_add_u32 and s_addc_u32 complete the address
        elif pc and re.match(r"s_addc?_u32 ", insn):
            insn, pc = re.sub(r",\s*\S+$", ", PCREL", insn), pc - 1
        cur.append(f"{int(m.group(2), 16) - base:x}: {insn}" + (f"   -> {m.group(3)}" if m.group(3) else ""))
    for lines in out.values():  # the padding up to the next kernel, or to the end of the section
        while lines and lines[-1].endswith(": s_nop 0"):
            lines.pop()
    return out


def build(lib):
    """({symbol: resource fields}, {symbol: [line]}) over every code object of lib."""
    rows, code = {}, {}
    for co in R.code_objects(lib):
        rows.update(R.kernels(co))
        code.update(disassembly(co))
    return rows, {name: code.get(name, []) for name in rows}


def main(argv):
    (rows_a, code_a), (rows_b, code_b) = build(argv[0]), build(argv[1])
    if "--rename" in argv:
        pattern, repl = argv[argv.index("--rename") + 1].split("=", 1)
        rows_a = {re.sub(pattern, repl, name): dict(row, name=re.sub(pattern, repl, row["name"]))
                  for name, row in rows_a.items()}
        code_a = {re.sub(pattern, repl, name): lines for name, lines in code_a.items()}
    diffs = 0
    for name in sorted(set(rows_a) ^ set(rows_b)):
        diffs += 1
        print(f"only in {argv[0] if name in rows_a else argv[1]}: {name}")
    for name in sorted(set(rows_a) & set(rows_b)):
        if rows_a[name] != rows_b[name]:
            diffs += 1
            print(f"resources differ: {name}\n  {rows_a[name]}\n  {rows_b[name]}")
        a, b = code_a[name], code_b[name]
        lines = [(x, y) for x, y in zip(a, b) if x != y]
        if lines or len(a) != len(b):
            diffs += 1
            print(f"code differs: {name}: {len(lines)} of {len(a)} lines, {len(b)} lines in the second")
            for x, y in lines[:5]:
                print(f"  - {x}\n  + {y}")
    print(f"{len(rows_a)} and {len(rows_b)} kernels, {sum(map(len, code_a.values()))} and "
          f"{sum(map(len, code_b.values()))} instructions: {diffs} differences")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

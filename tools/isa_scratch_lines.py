"""Where the certified f32 game kernels touch scratch, by source line.

Builds pg_relu.hip, pg_relu2.hip, pg_sig2.hip, pg_relu3.hip and pg_sig3.hip's device objects with line
tables (the product's flags plus -gline-tables-only), disassembles every game
kernel whose name contains SUBSTRING (default "_adv": the PG_KERNEL_ADVANCE
instances) and reports, per kernel, its scratch_* instructions by the source
line they belong to -- so that one can see that none sits on the frame's common
path (cert_game's own lines in pg_certgame.hpp, Pong::step, the f32 chain and
the certificate), DESIGN.md 4.2h.  Each unit is built twice, the second time
with -DPG_SOLO_UNIT as pong_amd/build.py does, so "_solo" lists the
PG_KERNEL_SOLO instances.  Needs no GPU.

    python tools/isa_scratch_lines.py [SUBSTRING] > listing.txt
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "neuro-genetic-pong-self-play_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
UNITS = [(u, f) for u in ("pg_relu.hip", "pg_relu2.hip", "pg_sig2.hip", "pg_relu3.hip", "pg_sig3.hip") for f in ((), ("-DPG_SOLO_UNIT",))]


def listing(tmp, unit, flags):
    obj = os.path.join(tmp, unit + ".o")
    subprocess.check_call([HIPCC, *flags, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fno-slp-vectorize", "-I", os.path.join(REPO, "include"), "-gline-tables-only",
                           "--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", obj, os.path.join(CSRC, unit)])
    return subprocess.check_output([OBJDUMP, "-d", "-l", "--no-show-raw-insn", obj], text=True)


def main(argv):
    want = argv[0] if argv else "_adv"
    total = collections.Counter()
    with tempfile.TemporaryDirectory() as tmp:
        for unit, flags in UNITS:
            sym, cur, rows = None, "?", {}
            for ln in listing(tmp, unit, flags).splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
                if m:
                    sym = m.group(1)
                    continue
                m = re.match(r"; (\S+):(\d+)", ln)
                if m:
                    cur = os.path.basename(m.group(1)) + ":" + m.group(2)
                    continue
                if sym and ln.startswith("\t") and re.match(r"\s*scratch_(load|store)", ln):
                    rows.setdefault(sym, collections.Counter())[(cur, ln.split()[0])] += 1
            names = sorted(rows)
            pretty = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
            for name, pn in zip(names, pretty):
                pn = re.sub(r"^void ", "", pn).replace("pg::", "").split("(")[0]
                if want not in pn.split("<")[0] or "decide" in pn:
                    continue
                print(f"# {pn}: {sum(rows[name].values())} scratch instructions")
                for (src, op), n in sorted(rows[name].items()):
                    print(f"  {n:4d} {op:22s} {src}")
                    total[src.split(":")[0]] += n
    print("# all listed kernels, scratch instructions by source file: " +
          ", ".join(f"{f} {n}" for f, n in total.most_common()))


if __name__ == "__main__":
    main(sys.argv[1:])

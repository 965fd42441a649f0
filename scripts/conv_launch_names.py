"""Replace the kernel handle offsets of a launchlog output by symbol names."""
import re
import subprocess
import sys

lib, log = sys.argv[1], sys.argv[2]
syms = {}
out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-t", lib], capture_output=True,
                     text=True, check=True).stdout
for line in out.splitlines():
    parts = line.split()
    if len(parts) >= 4 and re.fullmatch(r"[0-9a-f]{16}", parts[0]):
        name = parts[-1]
        if "__device_stub__" in name:
            continue
        syms.setdefault(int(parts[0], 16), name)
missing = 0
for line in open(log):
    m = re.match(r"  K ([0-9a-f]+) (.*)", line)
    if m:
        name = syms.get(int(m.group(1), 16))
        if name is None:
            missing += 1
            name = "?" + m.group(1)
        sys.stdout.write("  K %s %s\n" % (name, m.group(2)))
    else:
        sys.stdout.write(line)
sys.stderr.write("unnamed handles: %d\n" % missing)

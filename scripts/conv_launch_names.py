"""Replace the kernel handle offsets of a launchlog output by symbol names.

  conv_launch_names.py [--demangle | --short] libkcnn.so log

--demangle prints the demangled names, --short only the kernel's name with its
template arguments (conv_bwd_frame_kernel<1, true>): no return type, namespace or
parameter list.
"""
import re
import subprocess
import sys

args = sys.argv[1:]
mode = ""
if args and args[0] in ("--demangle", "--short"):
    mode = args.pop(0)
lib, log = args


def short(name):
    """'void ns::kern<1, true>(args)' -> 'kern<1, true>'."""
    depth, end = 0, len(name)
    for i, ch in enumerate(name):  # the parameter list: the first '(' outside <>
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and not name.startswith("(anonymous namespace)", i):
            end = i
            break
    name = name[:end]
    depth, start = 0, 0
    for i, ch in enumerate(name):  # after the last blank or '::' outside <>
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif depth == 0 and ch in " :":
            start = i + 1
    return name[start:]


syms = {}
out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-t"] + (["-C"] if mode else []) + [lib],
                     capture_output=True, text=True, check=True).stdout
for line in out.splitlines():
    parts = line.split()
    if len(parts) >= 4 and re.fullmatch(r"[0-9a-f]{16}", parts[0]):
        # "address flags section<TAB>size name": a demangled name has blanks
        name = parts[-1]
        if mode and "\t" in line:
            rest = line.split("\t", 1)[1].split(None, 1)
            name = rest[1] if len(rest) > 1 else ""
        if not name or "__device_stub__" in name:
            continue
        syms.setdefault(int(parts[0], 16), short(name) if mode == "--short" else name)
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

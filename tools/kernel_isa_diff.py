#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel, whatever unit a kernel lives in.

    for f in amira_amd/csrc/*.hip; do
      hipcc <CXXFLAGS of csrc/Makefile> --cuda-device-only -S $f -o DIR/$(basename $f .hip).s
    done                                   # once per tree, then:
    tools/kernel_isa_diff.py OLD_DIR NEW_DIR

For every kernel symbol (.amdhsa_kernel NAME) in either directory it takes the text from the symbol's
label to its .Lfunc_end: the instructions and the .amdhsa_kernel ... .end_amdhsa_kernel block (registers,
LDS, scratch).  It renames the labels that depend on a function's index in its unit (.LBB<n>_<m>, .Lfunc_end<n>),
drops comments and compares.  For a kernel that differs it also says whether the counts per opcode and the
descriptor's settings are equal: then the same instructions stand in another order.  Exit status 0: same kernel
names, no difference."""
import difflib
import pathlib
import re
import sys


def kernels(directory):
    """{mangled kernel name: normalised lines of its body + descriptor}"""
    out = {}
    for path in sorted(pathlib.Path(directory).glob("*.s")):
        lines = path.read_text().splitlines()
        for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M):
            body, state = [], 0  # 0: before the symbol's label, 1: inside, 2: .Lfunc_end seen
            for ln in lines:
                s = ln.split(";")[0].strip()  # (trailing comments name basic blocks by the function's index)
                if state == 0 and s == name + ":":
                    state = 1
                elif state == 1:
                    body.append(s)
                    if re.match(r"\.Lfunc_end\d+:", s):
                        state = 2
                        break
            # (the descriptor block sits inside that range, in .rodata between s_endpgm and .Lfunc_end)
            key = name + "@" + path.stem if name.startswith("_ZL") else name  # internal linkage: one per unit
            if state != 2 or ".end_amdhsa_kernel" not in body or key in out:
                sys.exit(f"{path}: kernel {name} is incomplete or defined twice")
            text = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", s)) for s in body]
            out[key] = [s for s in text if s]
    return out


def opcode_counts(body):
    """{mnemonic: how often} over the instructions (no labels, no directives)"""
    ops = [s.split()[0] for s in body if not s.startswith(".") and not s.endswith(":")]
    return {op: ops.count(op) for op in set(ops)}


def resources(body):
    """the descriptor's settings: registers, LDS, scratch and what else .amdhsa_kernel ... .end_amdhsa_kernel holds"""
    return [s for s in body if s.startswith(".amdhsa_") and not s.startswith(".amdhsa_kernel ")]


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = [k for k in sorted(set(old) & set(new)) if old[k] != new[k]]
    for k in only_old:
        print(f"only in {sys.argv[1]}: {k}")
    for k in only_new:
        print(f"only in {sys.argv[2]}: {k}")
    for k in differ:
        same_ops = opcode_counts(old[k]) == opcode_counts(new[k])
        same_res = resources(old[k]) == resources(new[k])
        print(f"differs: {k} ({len(old[k])} -> {len(new[k])} lines; counts per opcode "
              f"{'equal' if same_ops else 'DIFFER'}, descriptor resources {'equal' if same_res else 'DIFFER'})")
        for ln in list(difflib.unified_diff(old[k], new[k], "old", "new", lineterm="", n=1))[:40]:
            print("    " + ln)
    print(f"kernel_isa_diff: {len(old)} kernels old, {len(new)} new, {len(only_old)} only old, "
          f"{len(only_new)} only new, {len(differ)} differ")
    return 1 if only_old or only_new or differ else 0


if __name__ == "__main__":
    sys.exit(main())

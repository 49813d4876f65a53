#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files (hipcc --cuda-device-only -S) one by one.

usage: asm_kernel_diff.py OLD.s NEW.s

For each .amdhsa_kernel symbol: the instruction stream (comments stripped, function-local label numbers
normalised, since they count the functions before it in the file) and the .amdhsa_* descriptor block.  Prints
the symbols only one side has and the kernels whose text differs; exit status 0 when there are none.
"""
import re
import sys


def kernels(path):
    out, name, body, tail = {}, None, [], False
    for line in open(path):
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body, tail = m.group(1), [], False
            continue
        if name is None:
            continue
        if tail:  # behind the descriptor: the resource symbols it refers to (.set NAME.num_vgpr, ...)
            if line.strip().startswith(".set " + name + "."):
                out[name].append(line)
            continue
        if re.match(r"\s*\.(size|p2align|section|text|globl|protected|weak)\b", line):
            continue
        body.append(re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", line))
        if line.strip() == ".end_amdhsa_kernel":
            out[name] = body
            tail = True
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    diff = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print(f"{len(a)} kernels in {sys.argv[1]}, {len(b)} in {sys.argv[2]}")
    for k in only_a:
        print("only in old:", k)
    for k in only_b:
        print("only in new:", k)
    def desc(body):  # the descriptor block and the resource symbols behind it
        return body[next(i for i, x in enumerate(body) if x.strip().startswith(".amdhsa_kernel")):]

    for k in diff:
        n = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
        d = "same" if desc(a[k]) == desc(b[k]) else "DIFFERS"
        print(f"differs: {k} (old {len(a[k])} lines, new {len(b[k])}, first difference at line {n}; descriptor {d})")
    return 1 if only_a or only_b or diff else 0


if __name__ == "__main__":
    sys.exit(main())

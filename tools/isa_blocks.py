#!/usr/bin/env python3
"""Static instruction mix of one kernel, per basic block, from hipcc --save-temps assembly.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Ika9q_sdr_amd/csrc --save-temps -c ka9q_sdr_amd/csrc/kq_full16k.hip -o /tmp/x.o
  python3 tools/isa_blocks.py kq_full16k-hip-amdgcn-amd-amdhsa-gfx950.s k_filter_full16k [min_instructions] [--ops BLOCK]

Prints, for every basic block of at least `min_instructions`, the number of vector-ALU instructions (packed ones
separately), scalar, LDS and global-memory instructions.  With --ops BLOCK the opcode histogram of that block.
The dynamic count of a path is the sum over the blocks it runs through; compare with SQ_INSTS_VALU / SQ_WAVES.

  python3 tools/isa_blocks.py FILE.s KERNEL --path START DECISIONS

walks one executed path instead: from START (a block label, or `barrier:N` = behind the kernel's N-th s_barrier) to
s_endpgm, one letter of DECISIONS per conditional branch met (T taken, N falls through), and prints the branches with what
was decided and the vector instructions of the path by opcode.  (Loops: one letter per trip.)
"""
import collections
import re
import sys


def kernel_lines(path, name):
    out, on = [], False
    for ln in open(path):
        s = ln.strip()
        if not on:
            if re.match(r"^_Z\w*%s\w*:" % re.escape(name), s):
                on = True
            continue
        if s.startswith("s_endpgm"):
            # the last s_endpgm of the function ends it; .Lfunc_end follows
            out.append(s)
            continue
        if s.startswith(".Lfunc_end"):
            break
        out.append(s)
    return out


def walk(lines, start, decisions):
    """Instructions executed from `start` (a label, or `barrier:N` = behind the N-th s_barrier of the kernel, counted from 1)
    to s_endpgm.  Every conditional branch met consumes one letter of `decisions`: T taken, N not taken; s_branch is
    followed.  Returns (opcode histogram, [(branch line, target, letter)])."""
    labels = {}
    for i, s in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            labels[m.group(1)] = i
    if start.startswith("barrier:"):
        want, seen = int(start.split(":")[1]), 0
        for i, s in enumerate(lines):
            if s.startswith("s_barrier"):
                seen += 1
                if seen == want:
                    break
        else:
            raise SystemExit("fewer than %d barriers" % want)
        pc = i + 1
    else:
        pc = labels[start]
    ops, taken, d = collections.Counter(), [], list(decisions)
    while pc < len(lines):
        s = lines[pc]
        pc += 1
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        f = s.replace(",", " ").split()
        op = f[0]
        ops[op] += 1
        if op == "s_endpgm":
            break
        if op == "s_branch":
            pc = labels[f[1]]
        elif op.startswith("s_cbranch"):
            if not d:
                raise SystemExit("out of decisions at: " + s)
            letter = d.pop(0)
            taken.append((s, letter))
            if letter == "T":
                pc = labels[f[1]]
    if d:
        raise SystemExit("decisions left over: " + "".join(d))
    return ops, taken


def print_path(lines, start, decisions):
    ops, taken = walk(lines, start, decisions)
    for s, letter in taken:
        print("  %-40s %s" % (s, "taken" if letter == "T" else "falls through"))
    valu = {k: v for k, v in ops.items() if k.startswith("v_")}
    packed = sum(v for k, v in valu.items() if k.startswith("v_pk_"))
    print("executed path from %s [%s]: valu %d (packed %d) salu %d lds %d vmem %d" % (
        start, decisions, sum(valu.values()), packed, sum(v for k, v in ops.items() if k.startswith("s_")),
        sum(v for k, v in ops.items() if k.startswith("ds_")),
        sum(v for k, v in ops.items() if k.startswith(("global_", "buffer_", "flat_", "scratch_")))))
    for k, v in sorted(valu.items(), key=lambda kv: (-kv[1], kv[0])):
        print("    %-28s %d" % (k, v))


def main():
    path, name = sys.argv[1], sys.argv[2]
    args = sys.argv[3:]
    if "--path" in args:
        i = args.index("--path")
        print_path(kernel_lines(path, name), args[i + 1], args[i + 2])
        return
    ops_of = None
    if "--ops" in args:
        i = args.index("--ops")
        ops_of = args[i + 1]
        del args[i : i + 2]
    min_n = int(args[0]) if args else 25
    blocks = [["entry", collections.Counter()]]
    for s in kernel_lines(path, name):
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            blocks.append([m.group(1), collections.Counter()])
            continue
        if not s or s[0] in ";.":
            continue
        op = s.split()[0]
        blocks[-1][1][op] += 1
        if op.startswith(("s_cbranch", "s_branch")):  # the fall-through after a branch is a block of its own
            blocks.append(["%s+%d" % (blocks[-1][0].split("+")[0], len(blocks)), collections.Counter()])
    tot = collections.Counter()
    for name_, c in blocks:
        n = sum(c.values())
        cls = collections.Counter()
        for k, v in c.items():
            if k.startswith("v_pk_"):
                cls["pk"] += v
            if k.startswith("v_"):
                cls["valu"] += v
            elif k.startswith("s_"):
                cls["salu"] += v
            elif k.startswith("ds_"):
                cls["lds"] += v
            elif k.startswith(("global_", "buffer_", "flat_", "scratch_")):
                cls["vmem"] += v
        tot.update(cls)
        if ops_of == name_:
            for k, v in c.most_common():
                print("    %-28s %d" % (k, v))
        if n >= min_n and ops_of is None:
            print("%-12s total %5d  valu %5d (packed %4d)  salu %4d  lds %3d  vmem %3d" %
                  (name_, n, cls["valu"], cls["pk"], cls["salu"], cls["lds"], cls["vmem"]))
    if ops_of is None:
        print("whole kernel (static): valu %d (packed %d) salu %d lds %d vmem %d" %
              (tot["valu"], tot["pk"], tot["salu"], tot["lds"], tot["vmem"]))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Instruction counts of the 4-wide any-hit descent loop (ray_step's `if (quad) while (!(link & LEAF_BIT))`)
in one render_unified_kernel instance of `make asm`'s vrh_kernels.s.

    python tools/quad_loop_insts.py [visionaray_amd/_lib/asm/vrh_kernels.s] ["0, true, false, 6, 0, false, true, true"]
The second argument is a prefix of the instance's template arguments <KIND, AO, COUNT, OCC, EPI, LIST, BATCH,
SPILL, SAMPLED, SHARE> (default: the headline instance, AO with frames in flight and the overflow stack).

The loop is found by its loads: a 4-wide record is the only thing the kernel reads as seven 16-byte vector
loads, so each copy of the loop (ray_step<FAST = true> first, then FAST = false) is the loop -- the blocks the
compiler's "in Loop: Header=" comments give one header -- whose blocks hold exactly seven global_load_dwordx4.
The counts are static, one per instruction of those blocks: the cold blocks of an iteration (the overflow
store of a checked push, the restart on the binary records) are counted with the rest.
"""
import re
import subprocess
import sys


def functions(path):
    """mangled name -> list of lines of its body"""
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body = m.group(1), []
            out[name] = body
        elif name is not None:
            if ln.startswith("\t.end_amdhsa_kernel") or ln.startswith(".Lfunc_end"):
                name = None
            else:
                body.append(ln.rstrip("\n"))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return r[:len(names)]


def op_of(line):
    s = line.split(";", 1)[0].strip()
    if not s or s.endswith(":") or s.startswith("."):
        return None
    return s.split()[0]


BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)\s*(?:;\s*(.*))?$")


def blocks(body):
    """(label, loop comment, first line, last line) of every basic block"""
    out = []
    for i, ln in enumerate(body):
        m = BLOCK.match(ln)
        if m:
            if out:
                out[-1][3] = i - 1
            out.append([m.group(1) or "bb." + m.group(2), m.group(3) or "", i, len(body) - 1])
    return out


def loops(body):
    """the spans of the blocks of every loop whose blocks hold seven global_load_dwordx4 in all"""
    bl = blocks(body)
    found = []
    for lab, note, lo, hi in bl:
        if sum(1 for x in body[lo:hi + 1] if op_of(x) == "global_load_dwordx4") != 7:
            continue
        m = re.search(r"Header=(BB\d+_\d+)", note)
        head = m.group(1) if m else lab               # the block is the header itself, or names it
        spans = [(l, h) for la, no, l, h in bl if la == head or re.search(r"Header=%s\b" % head, no)]
        if sum(1 for l, h in spans for x in body[l:h + 1] if op_of(x) == "global_load_dwordx4") == 7:
            found.append(spans)
    return found


def count(body, spans):
    c = {"VALU": 0, "SALU": 0, "saveexec": 0, "branches": 0, "global_load_dwordx4": 0, "ds_write": 0,
         "ds_read": 0, "buffer": 0, "v_readlane": 0, "s_nop": 0, "s_waitcnt": 0}
    for ln in (x for lo, hi in spans for x in body[lo:hi + 1]):
        op = op_of(ln)
        if not op:
            continue
        if op == "s_branch" or op.startswith("s_cbranch"):
            c["branches"] += 1
        elif op in ("s_waitcnt", "s_nop"):
            c[op] += 1
        elif op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
            c["v_readlane"] += 1
            c["VALU"] += 1
        elif op.startswith("v_"):
            c["VALU"] += 1
        elif op.startswith("s_") and not op.startswith("s_load") and not op.startswith("s_buffer_load"):
            c["SALU"] += 1
            if "saveexec" in op:
                c["saveexec"] += 1
        elif op == "global_load_dwordx4":
            c[op] += 1
        elif op.startswith("ds_write"):
            c["ds_write"] += 1
        elif op.startswith("ds_read"):
            c["ds_read"] += 1
        elif op.startswith("buffer_"):
            c["buffer"] += 1
    return c


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else "visionaray_amd/_lib/asm/vrh_kernels.s"
    want = sys.argv[2] if len(sys.argv) > 2 else "0, true, false, 6, 0, false, true, true"
    fns = functions(path)
    names = [n for n in fns if "render_unified_kernel" in n]
    for n, d in zip(names, demangle(names)):
        args = d.split("render_unified_kernel<", 1)[1].split(">", 1)[0]
        if not args.startswith(want):
            continue
        found = loops(fns[n])
        print(f"<{args}>: {len(found)} copies of the 4-wide loop")
        for k, spans in enumerate(found):
            c = count(fns[n], spans)
            print(f"  copy {k} ({len(spans)} blocks): " + " ".join(f"{a} {b}" for a, b in c.items()))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Instruction order of K1's item blocks, read from device assembly (hipcc -S --cuda-device-only of csrc/corr_argmax.hip with
build.py's flags):  python tools/k1_item_order.py corr_argmax.s [substring of the kernel's demangled template arguments]

An item block is a basic block that holds 16 v_exp_f32 (in the kernel behind the FP6 screen, whose items open with the
tile maximum and branch to the exponentials: one that holds four v_mfma and no v_exp_f32).  One line per block, one letter per instruction:
  M v_mfma   E v_exp_f32   A v_add_f32   C v_cmp   X v_max3 / v_max   v other VALU   D ds_read   B buffer_load   n s_nop   w s_waitcnt
  b s_barrier   s other scalar
followed by the position of each MFMA among the block's VALU instructions (how many VALU instructions precede it), the
number of VALU instructions behind the last MFMA, and whether two MFMAs are adjacent.  profiles/k1_chain_order.txt is this
tool's output before and after the chain was spread."""
import re
import subprocess
import sys


def letter(op: str) -> str:
    if op.startswith("v_mfma"):
        return "M"
    if op.startswith("v_exp_f32"):
        return "E"
    if op.startswith("v_add_f32"):
        return "A"
    if op.startswith("v_cmp"):
        return "C"
    if op.startswith("v_max"):
        return "X"
    if op.startswith("v_"):
        return "v"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "D"
    if op.startswith("buffer_load"):
        return "B"
    if op == "s_nop":
        return "n"
    if op == "s_waitcnt":
        return "w"
    if op == "s_barrier":
        return "b"
    return "s"


def kernels(path):
    """{mangled name: [instruction lines and labels]} of every corr_bf16_direct_kernel in the file."""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w*corr_bf16_direct_kernel\w*):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        cur.append(line.rstrip("\n"))
    return out


def blocks(lines):
    """Basic blocks: cut at labels and behind branches."""
    blk = []
    for ln in lines:
        s = ln.strip()
        if not s or s.startswith(";") or s.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", s) and blk:
                yield blk
                blk = []
            continue
        op = s.split()[0]
        blk.append(op)
        if op.startswith("s_cbranch") or op == "s_branch" or op == "s_endpgm":
            yield blk
            blk = []
    if blk:
        yield blk


def describe(blk):
    s = "".join(letter(op) for op in blk[:-1] if not op.startswith("s_cbranch") and op != "s_branch") if blk else ""
    valu = "EACXv"
    pos, n = [], 0
    for ch in s:
        if ch == "M":
            pos.append(n)
        elif ch in valu:
            n += 1
    tail = n - pos[-1] if pos else n
    return s, pos, n, tail, "MM" in re.sub(r"[^M" + valu + r"]", "", s)


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else ""
    for name, lines in kernels(path).items():
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
        targs = re.search(r"corr_bf16_direct_kernel<([^>]*)>", dem)
        targs = targs.group(1) if targs else dem
        if want and want not in targs.replace(" ", ""):
            continue
        print(f"corr_bf16_direct_kernel<{targs}>")
        i = 0
        for blk in blocks(lines):
            nexp, nmf = (sum(op.startswith(k) for op in blk) for k in ("v_exp_f32", "v_mfma"))
            if not (nexp == 16 or (targs.replace(" ", "").endswith(",1") and nexp == 0 and nmf == 4)):
                continue
            s, pos, n, tail, adj = describe(blk)
            print(f"  {i:2d} {s}")
            print(f"     MFMA at VALU positions {pos} of {n}; VALU behind the last MFMA {tail}; adjacent MFMAs: {'yes' if adj else 'no'}")
            i += 1


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate zg_fips.h: the Fq / Fq2 add and sub forms of gfx950 (12 x 32-bit limbs), each a few
VALU carry chains in one inline-asm statement. Build tooling.

hipcc pads every inline-asm statement boundary with a wait state, and an instruction that reads a
carry mask (an SGPR pair) must not directly follow the one that writes it. So a whole form is one
statement and its independent chains are interleaved (schedule_chains below).

    python zebra_amd/csrc/gen_fips.py > zebra_amd/csrc/zg_fips.h
"""
import sys

N = 12


# ---------------------------------------------------------------- add / sub carry chains
# An Fq op is a few carry chains over 12 limbs plus per-limb selects. Instructions:
#   (text, reads_carry, writes_carry, chain_id, seq)   operands as %[name]
# The scheduler interleaves the chains of one statement so that no instruction reads a carry
# mask written by the instruction right before it (one wait state), inserting
# s_nop 0 only when nothing else is ready.
def op_add(tag, r, a, b):
    """r = (a + b) mod p: s = a + b ; d = s - p ; r = borrow ? s : d"""
    ins = []
    for i in range(N):
        x = "v_add_co_u32 %%[%ss%d], %%[%sk0], %s, %s" % (tag, i, tag, a(i), b(i)) if i == 0 else \
            "v_addc_co_u32 %%[%ss%d], %%[%sk0], %s, %s, %%[%sk0]" % (tag, i, tag, a(i), b(i), tag)
        ins.append((x, None if i == 0 else tag + "k0", tag + "k0", tag + "A", i, []))
    for i in range(N):
        x = "v_sub_co_u32 %s, %%[%sk1], %%[%ss%d], %%[p%d]" % (r(i), tag, tag, i, i) if i == 0 else \
            "v_subb_co_u32 %s, %%[%sk1], %%[%ss%d], %%[p%d], %%[%sk1]" % (r(i), tag, tag, i, i, tag)
        ins.append((x, None if i == 0 else tag + "k1", tag + "k1", tag + "B", i, []))
    for i in range(N):
        ins.append(("v_cndmask_b32 %s, %s, %%[%ss%d], %%[%sk1]" % (r(i), r(i), tag, i, tag), tag + "k1", None,
                    tag + "C", i, ["B%d" % (N - 1)]))
    return ins, ["%ss%d" % (tag, i) for i in range(N)], [tag + "k0", tag + "k1"]


def op_sub(tag, r, a, b):
    """r = (a - b) mod p: d = a - b ; e = d + p ; r = borrow ? e : d"""
    ins = []
    for i in range(N):
        x = "v_sub_co_u32 %s, %%[%sk0], %s, %s" % (r(i), tag, a(i), b(i)) if i == 0 else \
            "v_subb_co_u32 %s, %%[%sk0], %s, %s, %%[%sk0]" % (r(i), tag, a(i), b(i), tag)
        ins.append((x, None if i == 0 else tag + "k0", tag + "k0", tag + "A", i, []))
    for i in range(N):
        x = "v_add_co_u32 %%[%se%d], %%[%sk1], %s, %%[p%d]" % (tag, i, tag, r(i), i) if i == 0 else \
            "v_addc_co_u32 %%[%se%d], %%[%sk1], %s, %%[p%d], %%[%sk1]" % (tag, i, tag, r(i), i, tag)
        ins.append((x, None if i == 0 else tag + "k1", tag + "k1", tag + "B", i, []))
    for i in range(N):
        ins.append(("v_cndmask_b32 %s, %s, %%[%se%d], %%[%sk0]" % (r(i), r(i), tag, i, tag), tag + "k0", None,
                    tag + "C", i, ["B%d" % i, "A%d" % (N - 1)]))
    return ins, ["%se%d" % (tag, i) for i in range(N)], [tag + "k0", tag + "k1"]


def op_lzadd(tag, r, a, b):
    """r = a + b (no reduction)"""
    ins = []
    for i in range(N):
        x = "v_add_co_u32 %s, %%[%sk0], %s, %s" % (r(i), tag, a(i), b(i)) if i == 0 else \
            "v_addc_co_u32 %s, %%[%sk0], %s, %s, %%[%sk0]" % (r(i), tag, a(i), b(i), tag)
        ins.append((x, None if i == 0 else tag + "k0", tag + "k0", tag + "A", i, []))
    return ins, [], [tag + "k0"]


def op_psub(tag, r, a, b):
    """r = a - b (no reduction; the caller guarantees a >= b)"""
    ins = []
    for i in range(N):
        x = "v_sub_co_u32 %s, %%[%sk0], %s, %s" % (r(i), tag, a(i), b(i)) if i == 0 else \
            "v_subb_co_u32 %s, %%[%sk0], %s, %s, %%[%sk0]" % (r(i), tag, a(i), b(i), tag)
        ins.append((x, None if i == 0 else tag + "k0", tag + "k0", tag + "A", i, []))
    return ins, [], [tag + "k0"]


OPS = {"add": op_add, "sub": op_sub, "lzadd": op_lzadd, "psub": op_psub}


def schedule_chains(ops):
    """ops: list of (tag, instruction list). Dependencies: an instruction (chain X, limb i) needs
    (X, i-1) and the listed extra deps ('B5' = this op's chain B limb 5); a carry read must not
    directly follow its carry write."""
    pending = []
    for tag, ins in ops:
        for (txt, rc, wc, chain, i, deps) in ins:
            d = set()
            if i > 0:
                d.add((chain, i - 1))
            for dep in deps:
                d.add((tag + dep[0], int(dep[1:])))
            # chain B of add/sub/lzsub reads chain A's limb i
            if chain.endswith("B"):
                d.add((tag + "A", i))
            pending.append({"txt": txt, "rc": rc, "wc": wc, "id": (chain, i), "deps": d, "tag": tag})
    done, out, last_wc = set(), [], None
    while pending:
        left = {}
        for ins in pending:
            left[ins["tag"]] = left.get(ins["tag"], 0) + 1
        pick, best = None, -1
        for k, ins in enumerate(pending):  # ready, hazard-free, from the op with the most work left
            if ins["deps"] <= done and not (ins["rc"] is not None and ins["rc"] == last_wc):
                if left[ins["tag"]] > best:
                    pick, best = k, left[ins["tag"]]
        if pick is None:
            out.append("s_nop 0")
            last_wc = None
            continue
        ins = pending.pop(pick)
        out.append(ins["txt"])
        done.add(ins["id"])
        last_wc = ins["wc"]
    return out


def fq_ops_fn(name, kinds):
    """a device function computing len(kinds) independent Fq ops in one asm statement.
    Op j: r_j = kinds[j](a_j, b_j)."""
    ops, temps, carries = [], [], []
    for j, kd in enumerate(kinds):
        tag = "o%d" % j
        ins, tmp, car = OPS[kd](tag, lambda i, j=j: "%%[r%d_%d]" % (j, i), lambda i, j=j: "%%[a%d_%d]" % (j, i),
                                lambda i, j=j: "%%[b%d_%d]" % (j, i))
        ops.append((tag, ins))
        temps += tmp
        carries += car
    text = schedule_chains(ops)
    nops = sum(1 for t in text if t == "s_nop 0")
    args = ", ".join("uint32_t* r%d, const uint32_t* a%d, const uint32_t* b%d" % (j, j, j) for j in range(len(kinds)))
    outs = ['[r%d_%d] "=&v"(r%d[%d])' % (j, i, j, i) for j in range(len(kinds)) for i in range(N)]
    outs += ['[%s] "=&v"(tmp[%d])' % (t, k) for k, t in enumerate(temps)]
    outs += ['[%s] "=&s"(car[%d])' % (c, k) for k, c in enumerate(carries)]
    ins = ['[a%d_%d] "v"(a%d[%d])' % (j, i, j, i) for j in range(len(kinds)) for i in range(N)]
    ins += ['[b%d_%d] "v"(b%d[%d])' % (j, i, j, i) for j in range(len(kinds)) for i in range(N)]
    ins += ['[p%d] "v"(FQ_P[%d])' % (i, i) for i in range(N)]
    lines = ["// %s: %s (%d instructions, %d s_nop)" % (name, ", ".join(kinds), len(text) - nops, nops),
             "__device__ __forceinline__ void %s(%s) {" % (name, args),
             "  uint32_t tmp[%d];" % max(1, len(temps)), "  uint64_t car[%d];" % len(carries),
             # not volatile: a pure function of its operands (carries in explicit SGPR outputs, no
             # implicit vcc), so the compiler may issue the LDS loads of a lazy form ahead of it
             '  asm("%s"' % "\\n\\t".join(text),
             "               : " + ", ".join(outs),
             "               : " + ", ".join(ins) + ");", "}"]
    return lines


FQ_FNS = [("fqa_add", ["add"]), ("fqa_sub", ["sub"]), ("fqa_lzadd", ["lzadd"]),
          ("f2a_add", ["add", "add"]), ("f2a_sub", ["sub", "sub"]), ("f2a_lzadd", ["lzadd", "lzadd"]),
          ("f2a_sub_add", ["sub", "add"]),
          # plain (unreduced) accumulation steps of the staged engine's lazy operand forms
          ("f2p_as", ["lzadd", "psub"]), ("f2p_sa", ["psub", "lzadd"]), ("f2p_ss", ["psub", "psub"]), ("fqp_sub", ["psub"])]


def main():
    out = ["// GENERATED by zebra_amd/csrc/gen_fips.py -- do not edit.", "#pragma once"]
    out.append("// ---- Fq add / sub carry chains, one asm statement each (interleaved chains)")
    for name, kinds in FQ_FNS:
        out += fq_ops_fn(name, kinds)
    sys.stdout.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

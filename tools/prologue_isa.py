"""What K12's two C2 kernels do before their first useful loads go out, read off the instruction stream (CPU only).

    python tools/prologue_isa.py                      # the C2 kernels: tail <128,128,false|true>, fwd_bwd <8,8,true>
    python tools/prologue_isa.py 'fwd_bwd_kernel<16,16,true>' 'wgrad_adam_kernel<256,256,false>'
    python tools/prologue_isa.py 'fwd_bwd_lean_kernel<8,8,0,0>'      # the lean kernel <HTA, HTC, activation, head> (csrc/ppo_update_lean.hip)

Compiles csrc/ppo_update.hip, csrc/ppo_update_lean.hip and csrc/ppo_update_tail.hip (the units the named kernels live in) to gfx950 assembly in a temporary directory with csrc/build.py's
FLAGS (device side only) and, for every named kernel, prints
  (i)  the number of `s_waitcnt lgkmcnt(0)` before the first vector-memory instruction (kernel-argument and cursor
       round trips that nothing overlaps), and
  (ii) every `s_waitcnt vmcnt(N)` between the kernel's entry and its first `s_barrier`, with the number of vector loads
       issued before it (in text order: the stream is read straight through, the first dozen are listed).
A wave's vector loads retire in order, so `vmcnt(N)` lets only the youngest N stay in flight: a wait with N below the number
of loads issued after some load L is a wait for L.

Counts that a test asserts follow the branches (class Cfg: every path from the kernel's entry); the listing (ii) does not.
The checks of tests/test_k12_prologue_isa.py are functions here (tail_waits_before_operands, fwd_bwd_report).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from ppo_and_friends_amd.csrc import build as hip_build  # noqa: E402

# (first match wins: the lean kernel's name contains the general kernel's key)
UNITS = {"fwd_bwd_lean": "ppo_update_lean.hip", "fwd_bwd": "ppo_update.hip", "wgrad_adam": "ppo_update_tail.hip"}
DEFAULT_KERNELS = ("wgrad_adam_kernel<128,128,false>", "wgrad_adam_kernel<128,128,true>", "fwd_bwd_kernel<8,8,true>")

_VMEM = re.compile(r"^(global|buffer|flat|scratch)_(load|store|atomic)")
_VLOAD = re.compile(r"^(global|buffer|flat|scratch)_load")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")
_LGKM0 = re.compile(r"lgkmcnt\(0\)")


def have_hipcc():
    return os.path.exists(hip_build.HIPCC)


def compile_unit(source, out_dir):
    """csrc/<source> -> <out_dir>/<source>.s (device code only, build.py's flags); returns the path."""
    out = os.path.join(out_dir, source[:-4] + ".s")
    cmd = [hip_build.HIPCC, *hip_build.FLAGS, "--cuda-device-only", "-S", os.path.join(hip_build.HERE, source), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def mangled(kernel):
    """'fwd_bwd_kernel<8,8,true>' -> the fragment of the Itanium name that identifies the instantiation."""
    m = re.fullmatch(r"\s*(?:ppo_update_)?(\w+)<([^>]*)>\s*", kernel)
    if not m:
        raise ValueError(f"kernel name {kernel!r}: expected name<template arguments>")
    name = "ppo_update_" + m.group(1)
    args = ""
    for a in (x.strip() for x in m.group(2).split(",")):
        args += {"true": "Lb1E", "false": "Lb0E"}.get(a) or f"Li{int(a)}E"
    return f"{len(name)}{name}I{args}E"


def unit_of(kernel):
    for key, src in UNITS.items():
        if key in kernel:
            return src
    raise ValueError(f"kernel name {kernel!r}: not one of K12's fwd_bwd / fwd_bwd_lean / wgrad_adam kernels")


def kernel_text(asm_path, kernel):
    """The instructions of one kernel in text order: [(mnemonic, operands)]; a label is kept as ("label", name), a
    `; ppoaf_...` comment line as ("marker", text)."""
    tagm = mangled(kernel)
    out, inside = [], False
    with open(asm_path) as fh:
        for line in fh:
            if not inside:
                if line.startswith("_ZN5ppoaf") and tagm in line.split(":")[0]:
                    inside = True
                continue
            if line.strip().startswith("; ppoaf_"):            # a marker the source left (an asm statement of comment text)
                out.append(("marker", line.strip()[2:].strip()))
                continue
            s = line.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                break
            if s.endswith(":"):
                out.append(("label", s[:-1]))
            elif s and not s.startswith("."):
                parts = s.split(None, 1)
                out.append((parts[0], parts[1] if len(parts) > 1 else ""))
    if not out:
        raise KeyError(f"{kernel} ({tagm}) not found in {asm_path}")
    return out


class Cfg:
    """Basic blocks of a kernel's text and their successors (direct branches only: these kernels make no calls)."""

    def __init__(self, ins):
        self.blocks, self.succ, label_at = [[]], [], {}
        for op, args in ins:
            if op == "label":
                if self.blocks[-1]:
                    self.blocks.append([])
                label_at[args] = len(self.blocks) - 1
                continue
            self.blocks[-1].append((op, args))
            if op.startswith("s_cbranch") or op in ("s_branch", "s_endpgm"):
                self.blocks.append([])
        for i, blk in enumerate(self.blocks):
            op, args = blk[-1] if blk else ("", "")
            nxt = [i + 1] if i + 1 < len(self.blocks) else []
            if op == "s_endpgm":
                self.succ.append([])
            elif op == "s_branch":
                self.succ.append([label_at[args.strip()]])
            elif op.startswith("s_cbranch"):
                self.succ.append([label_at[args.strip()]] + nxt)
            else:
                self.succ.append(nxt)

    def fewest_waits_before(self, is_wait, is_target, start=(0, 0)):
        """Over every path from the kernel's entry (or from `start`, a (block, position)) to the first instruction
        `is_target` accepts on that path: the smallest
        number of instructions `is_wait` accepts ahead of it -- the waits no path there avoids -- and those waits.  (Blocks
        a branch can skip do not count: the text cannot tell which conditions exclude each other, and the longest path
        through it strings together blocks that no workgroup executes together.)  (None, []) if no path gets there."""
        memo, open_ = {}, set()

        def best(b):
            if b in memo:
                return memo[b]
            if b in open_:                                    # a loop that reaches no target adds nothing
                return None
            open_.add(b)
            seen, res = [], None
            for op, args in self.blocks[b][start[1] if b == start[0] else 0:]:
                if is_target(op, args):
                    res = seen
                    break
                if is_wait(op, args):
                    seen.append(f"{op} {args}")
            else:
                tails = [t for t in (best(s) for s in self.succ[b]) if t is not None]
                if tails:
                    res = seen + min(tails, key=len)
            open_.discard(b)
            memo[b] = res
            return res

        r = best(start[0])
        return (None, []) if r is None else (len(r), r)

    def find_all(self, pred):
        return [(b, i) for b, blk in enumerate(self.blocks) for i, (op, args) in enumerate(blk) if pred(op, args)]

    def waits_behind_sets(self, is_set, stop, start=(0, 0)):
        """Every path from the entry (or from `start`, a (block, position)) up to the first instruction `stop` accepts:
        the `s_waitcnt vmcnt(N)` that come behind a
        load `is_set` accepts, as (N, set loads issued so far on that path).  A path is followed until it issues some OTHER
        vector load behind a set load: from there on it waits for what it has just asked for (a dependent trip), which is
        not the question here.  Returns (waits, the set loads of the paths that reached `stop`)."""
        found, reached, seen = set(), set(), set()
        todo = [(start[0], 0, start[1])]
        while todo:
            b, sets, pos = todo.pop()
            if (b, sets) in seen:
                continue
            seen.add((b, sets))
            ended = False
            for op, args in self.blocks[b][pos:]:
                if stop(op, args):
                    reached.add(sets)
                    ended = True
                    break
                if _VLOAD.match(op):
                    if is_set(op, args):
                        sets += 1
                    elif sets:
                        ended = True
                        break
                elif sets and op == "s_waitcnt":
                    m = _VMCNT.search(args)
                    if m:
                        found.add((int(m.group(1)), sets))
            if not ended:
                todo.extend((s, sets, 0) for s in self.succ[b])
        return sorted(found), sorted(reached)


def _is_vmem(op, args):
    return bool(_VMEM.match(op))


def _is_lgkm0(op, args):
    return op == "s_waitcnt" and bool(_LGKM0.search(args))


def _is_vmcnt(op, args):
    return op == "s_waitcnt" and bool(_VMCNT.search(args))


def scalar_waits_before_vmem(ins):
    """(i): the `s_waitcnt lgkmcnt(0)` every path executes before its first vector-memory instruction."""
    return Cfg(ins).fewest_waits_before(_is_lgkm0, _is_vmem)


def vmcnt_waits_before_barrier(ins):
    """(ii) in text order: [(N, vector loads issued before)] for every `s_waitcnt vmcnt(N)` ahead of the first s_barrier of
    the text (branches not followed: the listing a reader of the assembly sees)."""
    out, loads = [], 0
    for op, args in ins:
        if op == "s_barrier":
            break
        if _VLOAD.match(op):
            loads += 1
        elif _is_vmcnt(op, args):
            out.append((int(_VMCNT.search(args).group(1)), loads))
    return out


_SOFFSET_REG = re.compile(r",\s*s\d+\s+offen")


def tail_waits_before_operands(ins):
    """Fused tail: the `s_waitcnt vmcnt` every path executes before the first operand load of a tile job.  The MFMA
    operands are read with `buffer_load_dword` and carry their row block in the scalar offset (`..., s25 offen`); the
    optimiser state has none (`..., 0 offen`, or plain global loads), the record traffic goes through 16-byte buffer loads.
    Paths that never reach an operand load (the idle workgroups, the output-segment jobs, the bookkeeping workgroup) do
    not count."""
    return Cfg(ins).fewest_waits_before(_is_vmcnt, lambda op, args: op == "buffer_load_dword" and bool(_SOFFSET_REG.search(args)))


MARK_TABLES = "ppoaf_rowtile_tables_prologue"


def fwd_bwd_report(ins):
    """fwd_bwd: scalar waits ahead of the first vector-memory instruction, and -- in the per-epoch-tables flavour of the
    row-tile body, which the source marks with a comment line where its requests begin (one per network) -- the vmcnt
    waits between the first hidden-set load (`buffer_load_dwordx4`: only the hidden weight sets are requested as 16-byte
    lines) and the S0 barrier, on any path.  A wait that allows fewer outstanding loads than the set loads issued so far
    waits for a hidden set."""
    n, which = scalar_waits_before_vmem(ins)
    cfg = Cfg(ins)
    waits, reached = set(), set()
    marks = cfg.find_all(lambda op, args: op == "marker" and args == MARK_TABLES)
    for m in marks:
        w, r = cfg.waits_behind_sets(lambda op, args: op == "buffer_load_dwordx4", lambda op, args: op == "s_barrier", start=m)
        waits.update(w)
        reached.update(r)
    waits = sorted(waits)
    return {"scalar_waits": n, "scalar_wait_list": which, "bodies": len(marks), "waits_after_first_set": waits,
            "set_loads_at_barrier": sorted(reached), "draining": [w for w in waits if w[0] < w[1]]}


# ---- the middle of the row-tile body (tests/test_k12_middle_isa.py): the head's row part, and the window between the barrier
#      that ends the head phase and the barrier that releases the hidden backward.  The TABLES flavour marks both.
MARK_HEAD_ROWS = ("ppoaf_rowtile_head_rows_begin", "ppoaf_rowtile_head_rows_end")
MARK_MIDDLE = ("ppoaf_rowtile_middle_begin", "ppoaf_rowtile_middle_end")
_GSTORE = re.compile(r"^(global|buffer|flat|scratch)_(store|atomic)")


def marked_windows(ins, marks):
    """Every instruction some path executes between a `marks[0]` line and the first `marks[1]` line behind it, one entry per
    begin marker: {"ins": [(op, args)], "closed": every path from the marker ends at an end marker (none runs into
    s_endpgm or into another begin marker first)}.  Branches are followed (class Cfg), so a block the compiler has laid out
    somewhere else in the text still counts."""
    cfg = Cfg(ins)
    begin, end = marks
    out = []
    for b0, i0 in cfg.find_all(lambda op, args: op == "marker" and args == begin):
        seen_ins, closed, visited = [], True, set()
        todo = [(b0, i0 + 1)]
        while todo:
            b, pos = todo.pop()
            if (b, pos) in visited:
                continue
            visited.add((b, pos))
            ended = False
            for op, args in cfg.blocks[b][pos:]:
                if op == "marker":
                    if args == end:
                        ended = True
                        break
                    if args == begin:
                        closed, ended = False, True
                        break
                    continue
                if op == "s_endpgm":
                    closed = False
                seen_ins.append((op, args))
            if not ended:
                todo.extend((s, 0) for s in cfg.succ[b])
        out.append({"ins": seen_ins, "closed": closed})
    return out


def middle_report(ins):
    """fwd_bwd, TABLES flavour: what the head's row part and the window behind the head's barrier contain that does not
    belong on the path to the hidden backward -- stores to global memory, cross-lane round trips through the LDS crossbar
    (`ds_bpermute` / `ds_permute`), and, for the window, barriers (it lies between two of them)."""
    def scan(marks):
        w = marked_windows(ins, marks)
        flat = [x for e in w for x in e["ins"]]
        return {"windows": len(w), "closed": all(e["closed"] for e in w), "instructions": len(flat),
                "global_stores": [f"{op} {args}" for op, args in flat if _GSTORE.match(op)],
                "permutes": [f"{op} {args}" for op, args in flat if op.startswith(("ds_bpermute", "ds_permute"))],
                "barriers": sum(op == "s_barrier" for op, _ in flat),
                "lds_writes": sum(op.startswith("ds_write") or op.startswith("ds_store") for op, _ in flat)}
    return {"head_rows": scan(MARK_HEAD_ROWS), "middle": scan(MARK_MIDDLE)}


# ---- the hidden forward layers of the row-tile body (tests/test_k12_hidden_isa.py).  The TABLES flavour marks the start of
#      the hidden forward, of each of its layers, the end of a layer's epilogue writes and the start of the hidden backward.
MARK_HIDDEN = ("ppoaf_rowtile_hidden_fwd_begin", "ppoaf_rowtile_hidden_bwd_begin")
MARK_LAYER = ("ppoaf_rowtile_hidden_layer_begin", "ppoaf_rowtile_hidden_epilogue_end")
_LDS_WRITE = re.compile(r"^ds_(write|store)")


def _reachable(cfg, start, stop):
    """Every (block, position) some path executes from `start` on, up to (not including) the first instruction on that
    path that `stop` accepts."""
    seen, todo = set(), [start]
    while todo:
        b, pos = todo.pop()
        while pos < len(cfg.blocks[b]) and (b, pos) not in seen and not stop(*cfg.blocks[b][pos]):
            seen.add((b, pos))
            pos += 1
        if pos == len(cfg.blocks[b]):
            todo.extend((s, 0) for s in cfg.succ[b] if (s, 0) not in seen)
    return seen


def _phase_of(cfg, start, stop):
    """{(block, position): barriers passed} for everything some path executes from `start` up to the first instruction
    `stop` accepts: which barrier-delimited phase an instruction belongs to (the fewest barriers, should paths disagree)."""
    phase, todo = {}, [(start[0], start[1], 0)]
    while todo:
        b, pos, n = todo.pop()
        while pos < len(cfg.blocks[b]) and phase.get((b, pos), 1 << 30) > n and not stop(*cfg.blocks[b][pos]):
            phase[(b, pos)] = n
            n += cfg.blocks[b][pos][0] == "s_barrier"
            pos += 1
        if pos == len(cfg.blocks[b]):
            todo.extend((s, 0, n) for s in cfg.succ[b])
    return phase


def kernel_scratch_bytes(asm_path, kernel):
    """`; ScratchSize: N` of the kernel's resource comment (bytes of scratch memory per lane)."""
    tagm, inside = mangled(kernel), False
    with open(asm_path) as fh:
        for line in fh:
            if not inside:
                inside = line.startswith("_ZN5ppoaf") and tagm in line.split(":")[0]
            elif line.startswith("; ScratchSize:"):
                return int(line.split(":")[1])
    raise KeyError(f"{kernel}: no ScratchSize line in {asm_path}")


def kernel_resource(asm_path, kernel, key):
    """`; <key>: N` of the kernel's resource comment, e.g. "NumVgprs", "TotalNumVgprs", "ScratchSize"."""
    tagm, inside = mangled(kernel), False
    with open(asm_path) as fh:
        for line in fh:
            if not inside:
                inside = line.startswith("_ZN5ppoaf") and tagm in line.split(":")[0]
            elif line.startswith(f"; {key}:"):
                return int(line.split(":")[1])
    raise KeyError(f"{kernel}: no {key} line in {asm_path}")


def instruction_count(ins):
    return sum(op not in ("label", "marker") for op, _ in ins)


def hidden_report(ins):
    """fwd_bwd, TABLES flavour, one entry per network:
      "late_loads": per hidden forward layer (in text order), the vector-memory loads that some path executes behind the
          layer's last MFMA and ahead of an LDS write of its epilogue -- a load from which an LDS write of the layer can be
          reached without passing an MFMA;
      "layer_mfmas": the MFMAs of each layer (a layer without any would make the line above empty for nothing);
      "dgrad_loads": the single-dword vector loads between the start of the hidden forward and the start of the hidden
          backward, the head's row part left out (its own loads are not weight requests), per barrier-delimited phase
          [hidden layer 1, hidden layer 2, output layer, head, output backward]: the two dgrad sets, which are the only
          weights this kernel fetches value by value."""
    cfg = Cfg(ins)
    is_mark = lambda name: (lambda op, args: op == "marker" and args == name)
    begins = cfg.find_all(is_mark(MARK_HIDDEN[0]))
    out = []
    for b0 in begins:
        window = _reachable(cfg, (b0[0], b0[1] + 1), is_mark(MARK_HIDDEN[1]))
        at = lambda p: cfg.blocks[p[0]][p[1]]
        head = set()
        for h in (p for p in window if is_mark(MARK_HEAD_ROWS[0])(*at(p))):
            head |= _reachable(cfg, (h[0], h[1] + 1), is_mark(MARK_HEAD_ROWS[1]))
        phase = _phase_of(cfg, (b0[0], b0[1] + 1), is_mark(MARK_HIDDEN[1]))
        by_phase = [0] * (max(phase.values()) + 1)
        for p in window - head:
            if re.match(r"^(global|buffer|flat)_load_dword$", at(p)[0]):
                by_phase[phase[p]] += 1
        late, mfmas = [], []
        for lb in sorted(p for p in window if is_mark(MARK_LAYER[0])(*at(p))):
            layer = _reachable(cfg, (lb[0], lb[1] + 1), is_mark(MARK_LAYER[1]))
            mfmas.append(sum(at(p)[0].startswith("v_mfma") for p in layer))
            bad = []
            for p in sorted(q for q in layer if _VLOAD.match(at(q)[0])):
                tail = _reachable(cfg, (p[0], p[1] + 1), lambda op, args: op.startswith("v_mfma") or is_mark(MARK_LAYER[1])(op, args))
                if any(_LDS_WRITE.match(at(q)[0]) for q in tail):
                    bad.append(" ".join(at(p)))
            late.append(bad)
        out.append({"layers": len(late), "late_loads": late, "layer_mfmas": mfmas, "dgrad_loads": by_phase})
    return out


def describe(kernel, ins):
    print(f"{kernel}: {instruction_count(ins)} instructions")
    n, _ = scalar_waits_before_vmem(ins)
    print(f"  (i)  s_waitcnt lgkmcnt(0) before the first vector-memory instruction (no path avoids them): {n}")
    waits = vmcnt_waits_before_barrier(ins)
    print(f"  (ii) s_waitcnt vmcnt(N) before the first s_barrier of the text: {len(waits)}")
    for n_out, loads in waits[:12]:
        print(f"         vmcnt({n_out}) after {loads} vector loads")
    if len(waits) > 12:
        print(f"         ... and {len(waits) - 12} more")
    if "wgrad_adam" in kernel:
        n, which = tail_waits_before_operands(ins)
        print(f"  vmcnt waits before the first operand load of a tile job: {n} {which}")
    if "fwd_bwd_kernel" in kernel or "fwd_bwd_lean_kernel" in kernel:
        r = fwd_bwd_report(ins)
        print(f"  row-tile bodies of the per-epoch-tables flavour: {r['bodies']}")
        print(f"  hidden-set loads in flight at the S0 barrier, by path: {r['set_loads_at_barrier']}")
        print(f"  vmcnt waits behind the first hidden-set load, up to the S0 barrier, as (N, set loads issued): "
              f"{r['waits_after_first_set']}")
        print(f"  of these, waits for a hidden set (N < set loads issued): {r['draining']}")
        for name, m in middle_report(ins).items():
            print(f"  {name}: {m['windows']} windows (closed: {m['closed']}), {m['instructions']} instructions, "
                  f"{len(m['global_stores'])} global stores, {len(m['permutes'])} ds_(b)permute, {m['barriers']} barriers")
        for i, h in enumerate(hidden_report(ins)):
            print(f"  hidden forward, network {i}: {h['layers']} layers of {h['layer_mfmas']} MFMAs, vector loads between a "
                  f"layer's last MFMA and its epilogue's LDS writes: {[len(x) for x in h['late_loads']]}; dgrad dword loads up "
                  f"to the hidden backward: {h['dgrad_loads']}")


def main(argv):
    kernels = argv or list(DEFAULT_KERNELS)
    if not have_hipcc():
        sys.exit(f"{hip_build.HIPCC} not found")
    with tempfile.TemporaryDirectory(prefix="ppoaf_isa_") as tmp:
        asm = {}
        for k in kernels:
            src = unit_of(k)
            if src not in asm:
                asm[src] = compile_unit(src, tmp)
            describe(k, kernel_text(asm[src], k))


if __name__ == "__main__":
    main(sys.argv[1:])

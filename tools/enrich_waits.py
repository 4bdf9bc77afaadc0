#!/usr/bin/env python3
"""Where does enrich_kernel wait for memory inside its tile loop?

Compiles binquant_amd/csrc/bq_enrich.hip to gfx950 assembly with the
Makefile's HIPFLAGS (device side only: no GPU is needed, hipcc is) and, for
every enrich_kernel instantiation, finds the tile loop — the depth-1 loop that
holds both workgroup barriers and the non-temporal output stores — and lists
every `s_waitcnt vmcnt(N)` inside it: the nearest memory instruction before
it, how many loads and stores were issued since the previous such wait, and
the instantiation's resource-usage line.

gfx950's vmcnt counts loads and stores alike, in order. vmcnt(0) inside the
loop therefore drains the tile's own output stores; a counted wait (N >= the
stores issued after the prefetch loads) lets them fly across the iteration.

Per tile loop it also reports the control flow (control_flow()): exec-mask
regions, how many of them hold an LDS access or an LDS read, exec-mask loops
(s_cbranch_execnz), the s_waitcnt that drain the LDS counter (lgkmcnt(0)) and
the instruction totals by class (VALU / SALU / LDS / VMEM / wait / branch).
An LDS read inside an exec-mask region can be neither hoisted out of it nor
batched with its neighbours: its round trip is waited for inside the region.

  python tools/enrich_waits.py                 # report on stdout
  python tools/enrich_waits.py --json          # the same as one JSON document
  python tools/enrich_waits.py --source FILE   # another revision of the kernel source

tests/test_enrich_waits.py and tests/test_enrich_straightline.py assert the
hot instantiation's properties from analyse().
"""

from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "binquant_amd", "csrc", "bq_enrich.hip")

_KERNEL = re.compile(r"^(_ZN2bq13enrich_kernelI(\w+?)EEvNS_10EnrichArgsEi):")
_LABEL = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)")
_IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
_THIS_HDR = re.compile(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=1\b")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")
_VMEM = re.compile(r"^\s+((?:global|flat|buffer|scratch)_(load|store|atomic)\w*)")


def hipcc_path() -> str | None:
    cand = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    if os.path.isfile(cand) and os.access(cand, os.X_OK):
        return cand
    return shutil.which("hipcc")


def makefile_hipflags() -> list[str]:
    """HIPFLAGS as the Makefile sets them (ARCH substituted)."""
    text = open(os.path.join(ROOT, "Makefile")).read().replace("\\\n", " ")
    var = {}
    for name in ("ARCH", "HIPFLAGS"):
        m = re.search(rf"^{name}\s*\?=\s*(.*)$", text, re.M)
        if not m:
            raise RuntimeError(f"Makefile: {name} not found")
        var[name] = m.group(1).strip()
    return var["HIPFLAGS"].replace("$(ARCH)", var["ARCH"]).split()


def compile_asm(source: str = SOURCE, hipcc: str | None = None) -> tuple[str, str]:
    """(device assembly, resource-usage remarks) of one kernel source."""
    hipcc = hipcc or hipcc_path()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bq_enrich.s")
        cmd = [hipcc, *makefile_hipflags(), "--cuda-device-only", "-S", source, "-o", out,
               "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stderr[-4000:]}")
        return open(out).read(), r.stderr


def resource_usage(remarks: str) -> dict[str, dict[str, int]]:
    """mangled kernel name -> {VGPRs, VGPRs Spill, SGPRs Spill, ScratchSize, LDS Size, Occupancy}"""
    res: dict[str, dict[str, int]] = {}
    cur = None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return res


def template_args(mangled_args: str) -> str:
    """'Lb0ELb1ELb1ELb1' -> 'DIV=0 VOUT=1 DEF=1 HOT=1' (HOT absent in older sources)"""
    bits = re.findall(r"Lb([01])E?", mangled_args + "E")
    names = ["DIV", "VOUT", "DEF", "HOT"]
    return " ".join(f"{n}={b}" for n, b in zip(names, bits))


def _kernels(asm: str):
    """(mangled, template args, body lines) per enrich_kernel instantiation"""
    lines = asm.splitlines()
    i = 0
    while i < len(lines):
        m = _KERNEL.match(lines[i])
        if not m:
            i += 1
            continue
        j = i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            j += 1
        yield m.group(1), m.group(2), lines[i + 1:j]
        i = j


def _loops(body: list[str]) -> dict[str, list[str]]:
    """depth-1 loop header -> the loop's instruction lines (nested loops
    included) in layout order, rotated so that the header's block comes first"""
    # a nested header names its depth-1 ancestor on its own or a following comment line
    parent: dict[str, str] = {}
    last_label = None
    for line in body:
        m = _LABEL.match(line)
        if m:
            last_label = m.group(1)
        elif not line.startswith(";"):
            last_label = None
        p = _PARENT.search(line)
        if p and last_label:
            parent.setdefault(last_label, p.group(1))
    loops: dict[str, list[str]] = {}
    start: dict[str, int] = {}
    cur = None
    for n, line in enumerate(body):
        m = _LABEL.match(line)
        if m:
            label = m.group(1)
            block = [line]
            k = n + 1
            while k < len(body) and body[k].startswith(";") and not _LABEL.match(body[k]):
                block.append(body[k])   # the header comment continues on the next lines
                k += 1
            text = " ".join(block)
            cur = None
            h = _THIS_HDR.search(text)
            il = _IN_LOOP.search(text)
            if h and label:
                cur = label if h.group(1) == "1" else parent.get(label)
                if h.group(1) == "1":
                    start[label] = len(loops.setdefault(label, []))
            elif il:
                cur = il.group(1) if il.group(2) == "1" else parent.get(il.group(1))
            if cur:
                loops.setdefault(cur, [])
            continue
        if cur and line.startswith("\t") and not line.lstrip().startswith((";", ".")):
            loops[cur].append(line)
    return {h: ls[start.get(h, 0):] + ls[:start.get(h, 0)] for h, ls in loops.items()}


def _is_nt_store(line: str) -> bool:
    return "global_store" in line and re.search(r"\bnt\b", line.split(";")[0]) is not None


def tile_loop(body: list[str]) -> tuple[str, list[str]] | None:
    """the depth-1 loop holding both barriers and the non-temporal stores (the
    VOUT=0 kernels store element-wise and temporal: there, the output stores)"""
    best = None
    for header, ls in _loops(body).items():
        barriers = sum("s_barrier" in x for x in ls)
        score = (sum(_is_nt_store(x) for x in ls), sum("global_store" in x for x in ls))
        if barriers >= 2 and score[1] and (best is None or score > best[2]):
            best = (header, ls, score)
    return (best[0], best[1]) if best else None


_SAVEEXEC = re.compile(r"^\s+s_(?:and|andn2|or|xor|orn2|nand|nor|xnor)_saveexec_b64\b")
_EXEC_NARROW = re.compile(r"^\s+s_mov_b64 exec, s")   # a mask formed outside the loop (hoisted condition)
_EXEC_RESTORE = re.compile(r"^\s+s_or_b64 exec, exec,")
_LGKM0 = re.compile(r"lgkmcnt\(0\)")


def control_flow(ls: list[str]) -> dict:
    """exec-mask regions, exec loops, LDS waits and instruction classes of a
    loop's instruction lines. Instructions are classed by the prefix of their
    mnemonic (v_: VALU, ds_: LDS, global_/flat_/buffer_/scratch_: VMEM,
    s_waitcnt and s_nop: wait, s_cbranch / s_branch: branch, any other s_:
    SALU); only the mnemonics counted here are named.

    An exec-mask region opens at an s_*_saveexec_b64 (or at an
    `s_mov_b64 exec, <mask>`, the form a loop-invariant condition takes) and
    closes at the next
    `s_or_b64 exec, exec, <saved>` of its nesting level, in layout order; the
    s_andn2_saveexec_b64 / s_or_saveexec_b64 that turns an if-part into its
    else-part continues the region. A region holds an LDS access (read) if a ds_ (ds_read) instruction
    lies inside it or inside a region nested in it."""
    classes = {"VALU": 0, "SALU": 0, "LDS": 0, "VMEM": 0, "wait": 0, "branch": 0, "other": 0}
    fp64 = 0
    open_regions: list[list[bool]] = []   # per open region: holds an LDS [access, read]
    regions = with_lds = with_read = 0
    for line in ls:
        code = line.split(";")[0]
        op = code.split()[0] if code.split() else ""
        if op.startswith("v_"):
            classes["VALU"] += 1
            fp64 += op.endswith("_f64") or "_f64_" in op
        elif op.startswith("ds_"):
            classes["LDS"] += 1
            open_regions = [[True, r or op.startswith("ds_read")] for _, r in open_regions]
        elif _VMEM.match(code):
            classes["VMEM"] += 1
        elif op in ("s_waitcnt", "s_nop"):
            classes["wait"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            classes["branch"] += 1
        elif op.startswith("s_"):
            classes["SALU"] += 1
        else:
            classes["other"] += 1
        if _SAVEEXEC.match(code) or _EXEC_NARROW.match(code):
            if op.startswith(("s_or_saveexec", "s_andn2_saveexec")) and open_regions:
                continue   # the else-part of the open region
            regions += 1
            open_regions.append([False, False])
        elif _EXEC_RESTORE.match(code) and open_regions:
            a, r = open_regions.pop()
            with_lds += a
            with_read += r
    with_lds += sum(a for a, _ in open_regions)
    with_read += sum(r for _, r in open_regions)
    return {"exec_regions": regions, "exec_regions_with_lds": with_lds, "exec_regions_with_lds_read": with_read,
            "saveexec": sum(1 for x in ls if _SAVEEXEC.match(x.split(";")[0])),
            "execz_branches": sum("s_cbranch_execz" in x.split(";")[0] for x in ls),
            "exec_loops": sum("s_cbranch_execnz" in x.split(";")[0] for x in ls),
            "waitcnt": sum("s_waitcnt" in x.split(";")[0] for x in ls),
            "lgkmcnt0_waits": sum(1 for x in ls if "s_waitcnt" in x.split(";")[0] and _LGKM0.search(x.split(";")[0])),
            "fp64_valu": fp64, "classes": classes}


def analyse(asm: str, remarks: str = "") -> list[dict]:
    usage = resource_usage(remarks)
    out = []
    for mangled, targs, body in _kernels(asm):
        rec = {"kernel": mangled, "template": template_args(targs), "resources": usage.get(mangled, {}),
               "code_lines": sum(1 for x in body if x.startswith("\t") and not x.lstrip().startswith((";", ".")))}
        tl = tile_loop(body)
        if tl is None:
            rec["tile_loop"] = None
            out.append(rec)
            continue
        header, ls = tl
        waits = []
        prev_op = None
        loads = stores = 0          # since the previous vmcnt wait
        seen_load = False           # a global load of this iteration already issued
        first_load = last_store = None
        n_loads = n_stores = n_nt = 0
        load_span_waits = 0         # vmcnt waits between the first and the last global load
        pending_span = 0
        for pos, line in enumerate(ls):
            code = line.split(";")[0]
            m = _VMEM.match(code)
            if m:
                prev_op = code.strip()
                if m.group(2) == "load":
                    loads += 1
                    if m.group(1).startswith("global"):
                        n_loads += 1
                        if seen_load:
                            load_span_waits += pending_span
                        pending_span = 0
                        seen_load = True
                        if first_load is None:
                            first_load = pos
                else:
                    stores += 1
                    if m.group(1).startswith("global"):
                        n_stores += 1
                        n_nt += _is_nt_store(line)
                        last_store = pos
                continue
            if "s_waitcnt" in code:
                v = _VMCNT.search(code)
                if v:
                    waits.append({"pos": pos, "vmcnt": int(v.group(1)), "text": code.strip(),
                                  "after": prev_op, "loads_since": loads, "stores_since": stores})
                    loads = stores = 0
                    if seen_load:
                        pending_span += 1
        # the prefetched tile is consumed from the loop header up to this
        # iteration's own prefetch, or (scheduled early) behind the last store
        for w in waits:
            w["guards_prefetch"] = ((first_load is None or w["pos"] < first_load)
                                    or (last_store is not None and w["pos"] > last_store))
        rec["tile_loop"] = {"header": header, "instructions": len(ls), "global_loads": n_loads,
                            "global_stores": n_stores, "nt_stores": n_nt,
                            "barriers": sum("s_barrier" in x for x in ls),
                            "scratch_ops": sum(1 for x in ls if re.match(r"\s+scratch_", x)),
                            "waits_between_prefetch_loads": load_span_waits, "waits": waits,
                            "control_flow": control_flow(ls)}
        out.append(rec)
    return out


def render(report: list[dict]) -> str:
    rows = []
    for rec in report:
        r = rec["resources"]
        rows.append(f"== enrich_kernel<{rec['template']}>")
        rows.append("   resources: " + ", ".join(f"{k} {r[k]}" for k in
                    ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize", "LDS Size", "Occupancy") if k in r)
                    + f"; {rec['code_lines']} instructions in the kernel")
        tl = rec["tile_loop"]
        if tl is None:
            rows.append("   no tile loop found")
            continue
        rows.append(f"   tile loop {tl['header']}: {tl['instructions']} instructions, {tl['global_loads']} global loads, "
                    f"{tl['global_stores']} global stores ({tl['nt_stores']} nt), {tl['barriers']} barriers, "
                    f"{tl['scratch_ops']} scratch ops; vmcnt waits between the first and last global load: "
                    f"{tl['waits_between_prefetch_loads']}")
        cf = tl["control_flow"]
        rows.append(f"   control flow: {cf['exec_regions']} exec-mask regions ({cf['exec_regions_with_lds']} holding an LDS "
                    f"access, {cf['exec_regions_with_lds_read']} an LDS read, {cf['saveexec']} saveexec, {cf['execz_branches']} execz branches), {cf['exec_loops']} exec loops "
                    f"(execnz); {cf['waitcnt']} s_waitcnt, {cf['lgkmcnt0_waits']} of them lgkmcnt(0)")
        rows.append("   instructions: " + ", ".join(f"{k} {v}" for k, v in cf["classes"].items())
                    + f"; fp64 VALU {cf['fp64_valu']}")
        for w in tl["waits"]:
            rows.append(f"   @{w['pos']:5d}  {w['text']:<34} after {w['after'] or '-':<60} "
                        f"(+{w['loads_since']} loads, +{w['stores_since']} stores"
                        f"{', guards the prefetched tile' if w['guards_prefetch'] else ''})")
    return "\n".join(rows) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default=SOURCE, help="kernel source to compile (default: the tree's bq_enrich.hip)")
    ap.add_argument("--asm", default=None, help="analyse this assembly file instead of compiling")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if args.asm:
        asm, remarks = open(args.asm).read(), ""
    else:
        asm, remarks = compile_asm(args.source)
    report = analyse(asm, remarks)
    sys.stdout.write(json.dumps(report, indent=1) + "\n" if args.json else render(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())

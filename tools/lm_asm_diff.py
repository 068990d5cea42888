#!/usr/bin/env python3
"""Compare the kernels of two device-only assembly listings of one HIP unit, by kernel name.

For a change that must leave the generated code alone (a refactor of the LM kernel's variant choice, say):
compile the unit at both revisions with the Makefile's FLAGS plus `--offload-device-only -S`, then

    tools/lm_asm_diff.py OLD.s NEW.s [OLD2.s NEW2.s ...]

Per kernel (and per device function that is not inlined) it compares the instructions (the function's text without comments, with the function index of the
local labels .LBB<i>_<n> / .Lfunc_end<i> / .LJTI<i>_<n> dropped, so the order of kernels in the file may differ), the
.amdhsa_kernel descriptor block and these fields of the metadata: .vgpr_count .agpr_count .sgpr_count
.vgpr_spill_count .sgpr_spill_count .private_segment_fixed_size .group_segment_fixed_size.
Prints per pair the kernel count and "identical", or the names that differ and in what; exit status 1 then."""
import re
import sys

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
          ".private_segment_fixed_size", ".group_segment_fixed_size")
LOCAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|Ltmp)\d+")


def kernels(path):
    """name -> dict(text=..., desc=..., meta={field: value}) of every function in the listing."""
    out, name, part, entry = {}, None, None, None
    for ln in open(path).read().splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            name, part = m.group(1), None
            out[name] = {"text": [], "desc": [], "meta": {}}
        elif name and ln.startswith(name + ":"):
            part = "text"
        elif re.match(r"\s*\.amdhsa_kernel\s", ln):  # (the descriptor stands inside the function's extent)
            part = "desc"
        elif ".end_amdhsa_kernel" in ln or re.match(r"\.Lfunc_end\d+:", ln):
            part = None if part == "desc" or ln.startswith(".Lfunc_end") else part
            name = None if ln.startswith(".Lfunc_end") else name
        elif part and ln.split(";")[0].strip():  # (comments dropped: they name loops by the function index too)
            out[name][part].append(LOCAL.sub(r".\1", ln.split(";")[0].strip()))
        if re.match(r"  - \.\w+:", ln):  # a kernel's entry of amdhsa.kernels (its arguments sit deeper)
            entry = {}
        m = re.match(r"  (?:- |  )(\.\w+):\s*(.*)", ln)
        if m and entry is not None:
            entry[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                out[m.group(2)]["meta"] = entry
    return out  # (kernels have a descriptor; the other entries are the device functions they call)


def main(argv):
    if len(argv) < 2 or len(argv) % 2:
        sys.exit(__doc__)
    bad = 0
    for old_path, new_path in zip(argv[0::2], argv[1::2]):
        old, new = kernels(old_path), kernels(new_path)
        diffs = [f"only in {old_path}: {k}" for k in sorted(set(old) - set(new))]
        diffs += [f"only in {new_path}: {k}" for k in sorted(set(new) - set(old))]
        for k in sorted(set(old) & set(new)):
            what = [w for w in ("text", "desc") if old[k].get(w) != new[k].get(w)]
            what += [f for f in FIELDS if old[k]["meta"].get(f) != new[k]["meta"].get(f)]
            assert not old[k]["desc"] or all(f in old[k]["meta"] for f in FIELDS), (k, old[k]["meta"])
            if what:
                diffs.append(f"{k}: {', '.join(what)}")
        n_old, n_new = (sum(1 for v in d.values() if v["desc"]) for d in (old, new))
        print(f"{old_path} vs {new_path}: {n_old} / {n_new} kernels, {len(old) - n_old} / {len(new) - n_new} device "
              "functions: " + ("identical" if not diffs else "DIFFER"))
        for d in diffs:
            print("  " + d)
        bad += len(diffs)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

#!/usr/bin/env python3
"""Compare two gfx950 device assemblies of the library kernel by kernel.

    hipcc <build_lib's flags without -shared> --cuda-device-only -S -o old.s 2d-gp_amd/csrc/gp2d.hip   (at the parent)
    hipcc ...                                                       -o new.s ...                      (at the change)
    python tools/asm_equal.py old.s new.s [-o profiles/NAME.json]

For every kernel (every `.amdhsa_kernel` block) it compares the function body, from the
function's label to its `.Lfunc_end`, and the `.amdhsa_*` resource directives, line by line.
Two things are normalised first: the mangled name of `igemm_nt_mod_kernel` is cut after its
<TBN, NST> arguments (a further template argument changes the rest of the name and nothing
else), and basic-block labels lose the function's running number.  It prints one verdict per
kernel and one JSON document; the exit status is 0 only when both files hold the same
kernels and all are equal."""
import argparse
import json
import re
import sys

IGEMM = re.compile(r"(_ZN4gp2d19igemm_nt_mod_kernelILi\d+ELi\d+E)\w*")
BLOCK = re.compile(r"\.LBB\d+_")


def norm(line):
    return BLOCK.sub(".LBB_", IGEMM.sub(r"\1", line)).strip()


def kernels(path):
    """name -> {"body": [...], "resources": [...]} for every kernel of one .s file."""
    lines = [norm(l) for l in open(path, encoding="utf-8", errors="replace")]
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"\.amdhsa_kernel\s+(\S+)$", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        j = i + 1
        while lines[j] != ".end_amdhsa_kernel":
            j += 1
        out[name] = {"resources": lines[i + 1:j]}
        i = j + 1
    for name, k in out.items():
        b = next(t for t, l in enumerate(lines) if l.startswith(name + ":"))
        e = next(t for t in range(b, len(lines)) if lines[t].startswith(".Lfunc_end"))
        k["body"] = lines[b + 1:e]
    return out


def resource(k, key):
    for l in k["resources"]:
        f = l.split()
        if f[0] == ".amdhsa_" + key:
            return int(f[1])
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-o", "--out", help="write the JSON document here too")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    rows = []
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            rows.append({"kernel": name, "verdict": "only in " + ("old" if name in old else "new")})
            continue
        o, n = old[name], new[name]
        row = {"kernel": name, "body_lines": len(o["body"]),
               "verdict": "equal" if o == n else "DIFFERENT"}
        if o != n:
            for part in ("body", "resources"):
                d = [(x, y) for x, y in zip(o[part], n[part]) if x != y]
                row[part + "_lines_old_new"] = [len(o[part]), len(n[part])]
                row[part + "_first_differences"] = d[:8]
        if "igemm_nt_mod_kernel" in name:
            row["new_resources"] = {k: resource(n, k) for k in
                                    ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size",
                                     "private_segment_fixed_size")}
        rows.append(row)
    equal = sum(r["verdict"] == "equal" for r in rows)
    doc = {"kernels": len(rows), "equal": equal, "all_equal": equal == len(rows), "per_kernel": rows}
    for r in rows:
        print(f'{r["verdict"]:>10}  {r["kernel"]}')
    print(f"{equal} of {len(rows)} kernels equal")
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if doc["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())

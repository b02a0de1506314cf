#!/usr/bin/env python3
"""Generates tests/golden/rust_items.json: for every `use knaster_*::...` line of the Rust shim and its golden-dump example
(bindings/rust/knaster_hip), the imported items that the knaster crates really declare in that module.

tests/test_abi.py checks the Rust sources against this file, so that the check needs no knaster sources at test time.
Run it against a checkout of the knaster workspace whenever a `use` line changes:

    python tests/golden/make_rust_items.py <knaster-workspace-dir>

An item is declared when its module file exists and holds `pub struct|enum|trait|fn|type|mod|const X` or re-exports X;
items the crates do not declare are reported and left out (the test then fails on them).
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
RUST = os.path.join(ROOT, "bindings", "rust", "knaster_hip")
SOURCES = ("examples/dump_golden.rs", "src/lib.rs")
CRATES = {"knaster_core": "knaster_core/src", "knaster_core_dsp": "knaster_core_dsp/src", "knaster_graph": "knaster_graph/src"}
USE_RE = r"^\s*use ((?:knaster_[a-z_]+)(?:::[a-z_0-9]+)*)::(\{[^}]*\}|[A-Za-z_0-9]+);"


def imports():
    """-> [(source, use path, [items])] for every knaster crate the shim imports from"""
    out = []
    for rel in SOURCES:
        src = open(os.path.join(RUST, rel)).read()
        for path, names in re.findall(USE_RE, src, flags=re.M):
            if path.split("::")[0] not in CRATES:
                continue
            out.append((rel, path, [n.strip().split(" as ")[0] for n in names.strip("{}").split(",") if n.strip()]))
    return out


def main(workspace: str) -> int:
    table, missing = {}, []
    for rel, path, items in imports():
        parts = path.split("::")
        crate, mods = parts[0], parts[1:]
        base = os.path.join(workspace, CRATES[crate])
        # the module's file: src/a/b.rs, src/a/b/mod.rs, or (crate root / re-exported `ugens::*`) anywhere below src/
        candidates = []
        if mods and mods[0] != "typenum":
            for stem in (os.path.join(base, *mods), os.path.join(base, "ugens", *mods)):
                candidates += [stem + ".rs", os.path.join(stem, "mod.rs")]
            candidates = [c for c in candidates if os.path.isfile(c)]
            if not candidates:
                missing.append(f"{rel}: no module file for {path} under {base}")
                continue
        else:
            # (knaster_core's root re-exports knaster_primitives wholesale: `pub use knaster_primitives::*`)
            for b in [base] + ([os.path.join(workspace, "knaster_primitives/src")] if crate == "knaster_core" else []):
                for d, _, files in os.walk(b):
                    candidates += [os.path.join(d, f) for f in files if f.endswith(".rs")]
        text = "\n".join(open(c).read() for c in candidates)
        entry = table.setdefault(path, [])
        for item in items:
            if mods and mods[0] == "typenum":  # a re-exported third-party crate: only that the re-export exists
                ok = re.search(r"pub use typenum|pub extern crate typenum|pub use [a-z_:]*typenum", text)
            else:
                ok = re.search(r"pub (?:struct|enum|trait|fn|type|mod|const|use [A-Za-z_0-9:{}, ]*)\s*\b%s\b" % re.escape(item), text)
            if ok:
                if item not in entry:
                    entry.append(item)
            else:
                missing.append(f"{rel}: `{item}` (use {path}::..) is not declared in the crate")
    for k in table:
        table[k].sort()
    with open(os.path.join(HERE, "rust_items.json"), "w") as f:
        json.dump(dict(sorted(table.items())), f, indent=1)
        f.write("\n")
    for m in missing:
        print(m, file=sys.stderr)
    return 1 if missing else 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))

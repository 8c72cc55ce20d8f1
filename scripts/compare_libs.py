"""Are two builds of libnazhip the same machine code?  For a source move that must change no kernel:

    python scripts/compare_libs.py <old.so> <new.so>

Compares the gfx950 kernel symbols, every kernel's instruction sequence (addresses relative to the
kernel's start), every kernel's code-object metadata (vgpr, agpr, sgpr, spills, scratch, LDS) and
the exported names (nm -D --defined-only, hipcc's per-unit __hip_cuid_ ids aside).  Exit status
0 = identical.  For an additive change (new kernels, new entry points, nothing existing touched):

    python scripts/compare_libs.py --allow-new <old.so> <new.so>

lists the kernels and exports that exist only in the new library without counting them; anything
missing from the new library, or different in both, still fails.
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tests.isa_ring import LLVM, code_objects, disassemble, functions  # noqa: E402

META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")


def metadata(co: bytes) -> dict:
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", f.name], capture_output=True, text=True,
                               check=True).stdout
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", notes)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", blk).group(1)
        vals = {"agpr_count": blk.split("\n", 1)[0].strip(": ")}
        for k in META:
            m = re.search(rf"\n    \.{k}:\s+(\S+)", blk)
            vals[k] = m.group(1) if m else None
        out[name] = vals
    return out


def kernels(lib: Path):
    """kernel symbol -> ([(relative address, instruction)], metadata)."""
    out = {}
    for co in code_objects(lib):
        meta = metadata(co)
        funcs = functions(disassemble(co))
        for name, vals in meta.items():
            start, insns = funcs[name]
            seq = [(a - start, t.split("//")[0].strip()) for a, t in insns]
            assert name not in out, f"{lib}: kernel {name} in two code objects"
            out[name] = (seq, vals)
    return out


def exports(lib: Path) -> list:
    r = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True)
    names = sorted(line.split()[-1] for line in r.stdout.splitlines() if line.strip())
    # (__hip_cuid_<hash>: hipcc's per-translation-unit id, a hash of the unit's path and options)
    return [n for n in names if not n.startswith("__hip_cuid_")]


def main() -> int:
    args = [a for a in sys.argv[1:] if a != "--allow-new"]
    allow_new = len(args) != len(sys.argv) - 1
    old, new = Path(args[0]), Path(args[1])
    ko, kn = kernels(old), kernels(new)
    bad = added = 0
    for name in sorted(set(ko) ^ set(kn)):
        print(f"kernel only in {'old' if name in ko else 'new'}: {name}")
        if allow_new and name in kn:
            added += 1
        else:
            bad += 1
    ninsn = 0
    for name in sorted(set(ko) & set(kn)):
        (so, mo), (sn, mn) = ko[name], kn[name]
        ninsn += len(sn)
        if mo != mn:
            print(f"metadata differs: {name}\n  old {mo}\n  new {mn}")
            bad += 1
        if so != sn:
            k = next((i for i, (x, y) in enumerate(zip(so, sn)) if x != y), min(len(so), len(sn)))
            print(f"code differs: {name}: {len(so)} vs {len(sn)} instructions, first at #{k}:"
                  f"\n  old {so[k] if k < len(so) else None}\n  new {sn[k] if k < len(sn) else None}")
            bad += 1
    eo, en = exports(old), exports(new)
    for name in sorted(set(eo) ^ set(en)):
        kind = "C++ export" if name.startswith("_Z") else "C export"  # the API is the C names (naz_hip.h)
        print(f"{kind} only in {'old' if name in eo else 'new'}: {name}")
        if allow_new and name in en:
            added += 1
        else:
            bad += 1
    same = "IDENTICAL" if not added else f"IDENTICAL where both exist, {added} additions"
    print(f"{old.name} vs {new.name}: {len(set(ko) & set(kn))} kernels ({ninsn} instructions), "
          f"{len(en)} exported names: {same if not bad else f'{bad} DIFFERENCES'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

"""Compare two device-assembly files of one translation unit kernel by kernel.

    hipcc <HIP_FLAGS without -shared> -S --cuda-device-only -I include -o a.s csrc/cbn_infer.hip
    python tools/compare_device_asm.py a.s b.s

A host-side refactor may change the order in which templates are instantiated,
and with it the order of the functions in the file and the function index the
compiler puts into local labels (.LBB<fn>_<n>, .Lfunc_end<fn>; the long-branch
labels .Lpost_getpc<n> are numbered through the whole file).  This splits
both files at their functions' .globl lines, drops comments, replaces that index,
and compares each function (code and kernel descriptor, up to
.end_amdhsa_kernel) and each entry of the metadata note by symbol name.
Exit status 0: the same symbols, each identical.
"""
import re
import sys


def functions(text):
    out, name, lines, done = {}, None, [], False
    for line in text.splitlines():
        m = re.match(r"\s*\.globl\s+(\S+)", line)
        if m and m.group(1).startswith("__hip_cuid"):  # the per-build id, then the metadata note (compared by entry)
            name = None
        elif m and not m.group(1).endswith(".kd"):
            name, lines, done = m.group(1), [], False
            out[name] = lines
        if name is None or done:
            continue
        line = re.sub(r"\s*;.*$", "", line)
        line = re.sub(r"\.L(BB|JTI|func_end|func_begin|tmp|post_getpc)\d+", r".L\1N", line)
        if line.strip():
            lines.append(line)
        done = ".end_amdhsa_kernel" in line
    return out


def metadata(text):
    start = text.find("amdhsa.kernels:")
    entries = re.split(r"\n  - ", text[start:text.find(".end_amdgpu_metadata", start)])[1:] if start >= 0 else []
    return {re.search(r"\.symbol:\s+(\S+)", e).group(1): e.split("\namdhsa.")[0] for e in entries if ".symbol:" in e}


def main(a, b):
    ta, tb = (re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(p).read()) for p in (a, b))
    bad = 0
    for what, fa, fb in (("function", functions(ta), functions(tb)), ("metadata entry", metadata(ta), metadata(tb))):
        for n in sorted(set(fa) | set(fb)):
            if n not in fa or n not in fb:
                print(f"{what} {n}: only in {a if n in fa else b}")
                bad += 1
            elif fa[n] != fb[n]:
                print(f"{what} {n}: differs")
                bad += 1
        print(f"{what}: {len(fa)} in {a}, {len(fb)} in {b}, {sum(len(v) for v in fa.values())} lines compared")
    print("identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

"""Registers, scratch and LDS of the conv-ensemble instantiations of the fc32 kernels against their two parents.
    make -C climateparameterizations.jl_amd/csrc asm && python tools/fc_conv_ens_resources.py climateparameterizations.jl_amd/csrc/_build/engine_fc.s

Reads the kernels' metadata entries of the device assembly (the figures tools/asm_same.py compares).  Each fc_{forward,adjoint}_conv_ens_kernel
instantiation is set beside the single conv handle's (fc_*_conv_kernel) and the plain ensemble's (fc_*_kernel<.., 16, .., ENS = true>) of the same
(NZ, TAPE, CA, RKC, SPLIT); exit status 1 when one exceeds the larger of the two in VGPRs, AGPRs, SGPRs, scratch, spills or static LDS."""
import re
import sys

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")


def kernels(path):
    out = {}
    for b in open(path).read().split("  - .agpr_count:")[1:]:
        b = ".agpr_count:" + b.split("\namdhsa.")[0]
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        out[name] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, b).group(1)) for f in FIELDS}
    return out


def targs(name, stem):
    m = re.match(r"_Z\d+%sI((?:L[ib]\d+E)+)E" % stem, name)
    return tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1))) if m else None


def main(path):
    ks = kernels(path)
    bad = 0
    print("%-9s %-22s %s" % ("kernel", "NZ TAPE CA RKC SPLIT", "  ".join("%-18s" % f[:18] for f in FIELDS)))
    for kind in ("forward", "adjoint"):
        conv = {targs(n, "fc_%s_conv_kernel" % kind): v for n, v in ks.items() if targs(n, "fc_%s_conv_kernel" % kind)}
        ens = {}
        for n, v in ks.items():
            t = targs(n, "fc_%s_kernel" % kind)
            if t and t[1] == 16 and len(t) == (7 if kind == "forward" else 6) and t[-1] == 1:      # <NZ, CW = 16, [TAPE,] CA, RKC, SPLIT, ENS = true>
                ens[(t[0],) + t[2:-1]] = v
        new = {targs(n, "fc_%s_conv_ens_kernel" % kind): v for n, v in ks.items() if targs(n, "fc_%s_conv_ens_kernel" % kind)}
        assert new and set(new) == set(conv) == set(ens), (len(new), len(conv), len(ens))
        for t in sorted(new):
            cells = []
            for f in FIELDS:
                a, c, e = new[t][f], conv[t][f], ens[t][f]
                over = a > max(c, e)
                bad += over
                cells.append("%-18s" % ("%d (%d, %d)%s" % (a, c, e, " !" if over else "")))
            print("%-9s %-22s %s" % (kind, " ".join(str(x) for x in t), "  ".join(cells)))
    print("each cell: conv ensemble (single conv handle, plain ensemble); %d figure(s) above the larger parent" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))

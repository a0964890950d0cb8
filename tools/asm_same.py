"""Are the kernels of two device-assembly files (make -C csrc asm) the same?  python tools/asm_same.py OLD.s NEW.s
Either side may be several files joined with commas (a translation unit that was split: OLD.s NEW_a.s,NEW_b.s): their kernels are taken together.

Compares per mangled kernel name, not per byte: the order in which the compiler emits template instantiations follows the
host code's references, and the function numbers inside local labels (.LBB12_3) follow that order.  Per kernel: the text from
its 'Begin function' to its 'End function' line (instructions and the .amdhsa_kernel descriptor: register counts, LDS and
scratch sizes), its .set lines and its metadata entry (spill counts, arguments), comments dropped, label numbers removed."""
import re, sys

def kernels(paths):
    s = "\n".join(open(p).read() for p in paths.split(','))
    out = {}
    for m in re.finditer(r'; -- Begin function (\S+)\n(.*?); -- End function', s, re.S):
        out[m.group(1)] = m.group(2)
    for m in re.finditer(r'^\s*\.set (\w+)\.(.*\n)', s, re.M):
        if m.group(1) in out: out[m.group(1)] += '.set ' + m.group(2)
    for b in s.split('  - .agpr_count:')[1:]:
        b = b.split('\namdhsa.')[0]
        out[re.search(r'\.name:\s+(\S+)', b).group(1)] += b
    norm = lambda t: [l for l in (re.sub(r'\.(LBB|Ltmp|Lfunc_begin|Lfunc_end|LJTI)\d+', r'.\1', l.split(';')[0]).strip() for l in t.split('\n')) if l]
    return {k: norm(v) for k, v in out.items()}

a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
for n in sorted(set(a) - set(b)): print('only in', sys.argv[1], n)
for n in sorted(set(b) - set(a)): print('only in', sys.argv[2], n)
diff = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
for n in diff: print('differs', n)
print('%d kernels in %s, %d in %s, %d in both, %d differing' % (len(a), sys.argv[1], len(b), sys.argv[2], len(set(a) & set(b)), len(diff)))
sys.exit(1 if diff or set(a) != set(b) else 0)

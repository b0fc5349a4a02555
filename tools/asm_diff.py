"""Compare two `make asm` outputs kernel by kernel (labels and comments normalised): SAME / DIFF / NEW per kernel.
A kernel template that gained trailing parameters renames its old instantiations (k<a, b> becomes k<a, b, false>; a kernel that became a
template, k becomes k<false>; one that gained a trailing parameter PACK keeps k<a, b> with the empty pack, under another symbol): such a
kernel is compared with the one it was and marked `+param`.
usage: python tools/asm_diff.py old.s new.s"""
import re, subprocess, sys

def funcs(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z[^\n:]*):[^\n]*\n(.*?)^\.Lfunc_end\d+:', s, re.S | re.M):
        body = re.sub(r';.*', '', m.group(2))
        body = re.sub(r'\.LBB\d+_\d+', 'LBB', body)
        out[m.group(1)] = [l.strip() for l in body.split('\n') if l.strip() and not l.strip().startswith('.')]
    return out

def dem(n):
    d = subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()
    m = re.search(r'(k_\w+(<[^>]*>)?)', d)
    return m.group(1) if m else d[:70]

def was(name, old_names):
    """the old name of a kernel whose template gained trailing `false` parameters or an empty parameter pack, or None"""
    d = dem(name)
    if d in old_names: return old_names[d]
    while True:
        d2 = re.sub(r'(, |<)false>$', lambda m: '>' if m.group(1) == ', ' else '', d)
        if d2 == d: return None
        d = d2
        if d in old_names: return old_names[d]

a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
print(len(a), 'kernels before,', len(b), 'after')
old_names = {dem(n): n for n in a if n not in b}
renamed = set()
for n in b:
    o = n if n in a else was(n, old_names)
    if o is not None:
        if o != n: renamed.add(o)
        va = sum(1 for l in a[o] if l.startswith('v_')); vb = sum(1 for l in b[n] if l.startswith('v_'))
        print('SAME' if a[o] == b[n] else 'DIFF', f'{len(a[o]):6d} {len(b[n]):6d}  valu {va:5d} {vb:5d} ', dem(n), '' if o == n else '+param')
    else:
        print('NEW ', f'{"":6s} {len(b[n]):6d}  valu {"":5s} {sum(1 for l in b[n] if l.startswith("v_")):5d} ', dem(n))
for n in a:
    if n not in b and n not in renamed: print('GONE', dem(n))

"""Compare two `make asm` outputs kernel by kernel (labels and comments normalised): SAME / DIFF / NEW per kernel.
A kernel template that gained trailing parameters renames its old instantiations (k<a, b> becomes k<a, b, false>; a kernel that became a
template, k becomes k<false>; one that gained a trailing parameter PACK keeps k<a, b> with the empty pack, under another symbol): such a
kernel is compared with the one it was and marked `+param`.  r20_name holds the one renaming that is no such growth: the surface pass's
eleven positional parameters became six named axes and the camera kernels one template over the camera kind.  r22_name: the denoiser's two
prep kernels became one template over the albedo source.  r30_name: the baked view's eight shells became one template over the ending's
axes (FIRST, GRID, VIS, SPEC, DIR), the grid lookup's two hooks one over VIS.
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

def r20_name(d):
    """the name since the variant axes of a kernel as named before them (demangled, as dem gives it), or d itself"""
    m = re.fullmatch(r'(k_\w+?)(?:<(.*)>)?', d)
    k, t = m.group(1), (m.group(2).split(', ') if m.group(2) else [])
    u = lambda i: f'{i}u'
    on = lambda x: x == 'true'
    if k == 'k_shade_surface' and len(t) == 11:
        q, vol, inl, ident, lst, lens, rays, tex, one, em, nm = [t[0]] + [on(x) for x in t[1:]]
        surface = 0 if not tex else (4 if em else 3) if nm else (2 if em else 1)
        axes = [int(vol), (2 if ident else 1) if inl else 0, 2 if rays else int(lst), (2 if one else 1) if lens else 0, surface]
        return f'{k}<{", ".join([q] + [u(x) for x in axes])}>'
    cam = {'k_generate': ('0u', 'false'), 'k_generate_list': ('0u', 'true'), 'k_guide_rays': ('0u',), 'k_guide_rays_lens': ('1u',)}
    if d in cam: return f'{k.replace("_list", "").replace("_lens", "")}<{", ".join(cam[d])}>'
    if k == 'k_generate_lens': return f'k_generate<1u, {t[0]}>'
    if k == 'k_generate_proj': return f'k_generate<{u(int(t[1][:-1]) + 1)}, {t[0]}>'          # PROJ_PANORAMA 1, PROJ_ORTHOGRAPHIC 2 -> CAM_PANORAMA 2, CAM_ORTHOGRAPHIC 3
    if k == 'k_guide_rays_proj': return f'k_guide_rays<{u(int(t[0][:-1]) + 1)}>'
    if k == 'k_accumulate' and len(t) == 5:
        view = 'pt::CameraProjView' if on(t[4]) else 'pt::CameraLensView' if on(t[3]) else 'pt::CameraView'
        return f'{k}<{", ".join([view] + t[:3])}>'
    return d

def r22_name(d):
    """the merged prep kernel's name for k_dn_prep and k_dn_prep_albedo<MEAN> (AlbedoFrom: None 0, Image 1, Sums 2), or d itself"""
    src = {'k_dn_prep': 0, 'k_dn_prep_albedo<false>': 1, 'k_dn_prep_albedo<true>': 2}
    return f'k_dn_prep<(pt::(anonymous namespace)::AlbedoFrom){src[d]}>' if d in src else d

def r30_name(d):
    """the one baked kernel's instantiation for a shell of the baked view as named before the ending's axes, or d itself"""
    if d == 'k_probe_grid_lookup_vis': return 'k_probe_grid_lookup<true>'
    m = re.fullmatch(r'k_baked_follow_(probes|probes_vis|probes_spec|probes_spec_vis|dir|probes_dir|probes_spec_dir)<(\w+)(?:, (\w+))?>', d)
    if not m: return d
    shell, first, vis = m.groups()
    axes = ['true' if 'probes' in shell else 'false', vis or ('true' if 'vis' in shell else 'false'), 'true' if 'spec' in shell else 'false', 'true' if 'dir' in shell else 'false']
    return f'k_baked_follow<{", ".join([first] + axes)}>'

a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
print(len(a), 'kernels before,', len(b), 'after')
old_names = {r30_name(r22_name(r20_name(dem(n)))): n for n in a if n not in b}
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

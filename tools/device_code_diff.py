"""Compare the gfx950 device assembly of two trees kernel by kernel (kernels may change units).

    python tools/device_code_diff.py PARENT_DIR NEW_DIR | c++filt

Each directory holds one NAME.hip.s per source, from
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math --cuda-device-only -S
Per kernel symbol: the instruction text, the .amdhsa_kernel descriptor and the metadata entry,
less what only numbers the unit (comments, function indices in local labels, the unit id).
Prints the kernels that differ, that are gone or new, and whose number of copies changed.
"""
import re, sys, glob, os, collections

def kernels(path):
    """{kernel symbol: (body text, descriptor text, metadata text)} of one .s file."""
    txt = open(path).read()
    lines = txt.split('\n')
    out = {}
    # descriptors
    desc = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', txt, re.S):
        desc[m.group(1)] = m.group(2)
    # metadata entries: split the yaml's kernel list on '  - .agpr_count' style items
    meta = {}
    mm = re.search(r'amdhsa\.kernels:\n(.*?)\namdhsa\.target', txt, re.S)
    if mm:
        items = re.split(r'\n  - ', '\n' + mm.group(1))
        for it in items:
            n = re.search(r'\.name:\s+(\S+)', it)
            if n:
                meta[n.group(1)] = it
    for sym in desc:
        # body: from "sym:" label to ".Lfunc_end"
        m = re.search(r'^%s:.*?\n(.*?)^\.Lfunc_end\d+:' % re.escape(sym), txt, re.S | re.M)
        body = m.group(1) if m else ''
        out[sym] = (body, desc[sym], meta.get(sym, ''))
    return out

def norm(s):
    s = re.sub(r'\.LBB\d+_', '.LBB_', s)
    s = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', s)
    s = re.sub(r'__hip_cuid_\w+', '__hip_cuid', s)
    s = re.sub(r'\.Ltmp\d+', '.Ltmp', s)
    s = re.sub(r'[ \t]*;.*$', '', s, flags=re.M)  # comments (they carry function-numbered block names)
    s = re.sub(r'\n\s*\n', '\n', s)
    return s

def load(d):
    allk = collections.defaultdict(list)
    for p in sorted(glob.glob(os.path.join(d, '*.s'))):
        for sym, v in kernels(p).items():
            allk[sym].append((os.path.basename(p), tuple(norm(x) for x in v)))
    return allk

a, b = load(sys.argv[1]), load(sys.argv[2])
print('kernels (distinct symbols): parent %d, new %d; copies: parent %d, new %d' % (len(a), len(b), sum(map(len, a.values())), sum(map(len, b.values()))))
bad = 0
for sym in sorted(set(a) | set(b)):
    if sym not in b:
        print('GONE    %s  (parent: %s)' % (sym, ', '.join(u for u, _ in a[sym])))
        continue
    if sym not in a:
        print('NEW     %s  (new: %s)' % (sym, ', '.join(u for u, _ in b[sym])))
        continue
    va = {v for _, v in a[sym]}
    vb = {v for _, v in b[sym]}
    if len(va) != 1 or len(vb) != 1:
        # copies differing among themselves in one tree: compare per unit
        da = dict(a[sym]); db = dict(b[sym])
        for u in sorted(set(da) | set(db)):
            if u in da and u in db and da[u] != db[u]:
                bad += 1; print('DIFF    %s in %s' % (sym, u))
        if len(va) != 1: print('note: parent copies of %s differ among units (%d forms)' % (sym, len(va)))
        if not vb <= va:
            bad += 1; print('DIFF    %s: a new form matches no parent form' % sym)
        continue
    if va != vb:
        bad += 1
        print('DIFF    %s' % sym)
    if len(a[sym]) != len(b[sym]):
        print('COPIES  %s  parent %d (%s) -> new %d (%s)' % (sym, len(a[sym]), ', '.join(u for u, _ in a[sym]), len(b[sym]), ', '.join(u for u, _ in b[sym])))
print('differing kernels: %d' % bad)

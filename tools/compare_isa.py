#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libfmgan_hip.so: kernel set, resource metadata and instruction streams.

For a refactor that must not move a single instruction.  No GPU and no recompilation: the code objects are extracted
from each library (llvm-objdump --offloading), the kernels listed with their metadata (llvm-readelf --notes) and
disassembled (llvm-objdump -d).  Addresses, encodings and symbol names are normalised away; what is left of a kernel —
its instruction sequence with every operand and every relative branch distance — must be identical.

    tools/compare_isa.py OLD.so NEW.so [--rename MAP.json] [--md REPORT.md]

MAP.json is a list of [old fragment, new fragment] pairs applied to the OLD kernel names (a kernel whose template
parameters were renamed).  A kernel of OLD without a partner in NEW is reported as removed, one of NEW without a
partner as added.  Exit status 1 if a kernel that stays differs in metadata or instructions, or if one was added.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin')
META = ('.vgpr_count', '.sgpr_count', '.vgpr_spill_count', '.private_segment_fixed_size', '.group_segment_fixed_size')


def kernels_of(lib):
    """{kernel name: (metadata dict, [normalised instruction, ...])} over every gfx950 code object of the library."""
    objdump, readelf = os.path.join(LLVM, 'llvm-objdump'), os.path.join(LLVM, 'llvm-readelf')
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, 'lib.so'))
        subprocess.run([objdump, '--offloading', 'lib.so'], check=True, capture_output=True, cwd=d)
        for f in sorted(os.listdir(d)):
            if not f.endswith('gfx950'):
                continue
            path = os.path.join(d, f)
            notes = subprocess.run([readelf, '--notes', path], check=True, capture_output=True, text=True).stdout
            meta = {}
            for blk in notes.split('- .agpr_count')[1:]:
                name = re.search(r'\.name:\s+(\S+)', blk).group(1)
                meta[name] = {k: int(re.search(re.escape(k) + r':\s+(\d+)', blk).group(1)) for k in META}
            asm = subprocess.run([objdump, '-d', '--no-show-raw-insn', path], check=True, capture_output=True,
                                 text=True).stdout
            body = {}
            cur = None
            for line in asm.splitlines():
                m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
                if m:
                    cur = body.setdefault(m.group(1), []) if m.group(1) in meta else None
                    continue
                if cur is None or not line.strip():
                    continue
                ins = line.split('//')[0].strip()        # drop the address / encoding comment
                ins = re.sub(r'<[^>]*>', '<sym>', ins)   # symbolised targets: names differ, distances are operands
                if ins and ins != '...':                 # '...': zero padding between two functions
                    cur.append(ins)
            for name in meta:
                assert name not in out, f'{name} defined twice in {lib}'
                out[name] = (meta[name], body.get(name, []))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--rename', help='JSON list of [old fragment, new fragment] applied to OLD kernel names')
    ap.add_argument('--md', help='write the summary as markdown to this file')
    a = ap.parse_args()
    pairs = json.load(open(a.rename)) if a.rename else []
    old, new = kernels_of(a.old), kernels_of(a.new)

    def renamed(n):
        for frm, to in pairs:
            if frm in n:
                return n.replace(frm, to)
        return n

    same, differ, removed = [], [], []
    seen = set()
    for n in sorted(old):
        m = renamed(n)
        if m not in new:
            removed.append(n)
            continue
        seen.add(m)
        (mo, io), (mn, inn) = old[n], new[m]
        why = []
        if mo != mn:
            why.append('metadata ' + ', '.join(f'{k} {mo[k]} -> {mn[k]}' for k in META if mo[k] != mn[k]))
        if io != inn:
            first = next((i for i, (x, y) in enumerate(zip(io, inn)) if x != y), min(len(io), len(inn)))
            why.append(f'instructions {len(io)} -> {len(inn)}, first difference at #{first}')
        if not io:
            why.append('no disassembly found')
        (differ if why else same).append((n, m, '; '.join(why)))
    added = sorted(set(new) - seen)

    lines = ['| | count |', '|---|---|',
             f'| kernels in the old library | {len(old)} |', f'| kernels in the new library | {len(new)} |',
             f'| compared (present in both, under the name mapping) | {len(same) + len(differ)} |',
             f'| identical: metadata ({", ".join(k[1:] for k in META)}) and instruction sequence | {len(same)} |',
             f'| different | {len(differ)} |', f'| removed | {len(removed)} |', f'| added | {len(added)} |', '']
    n_ins = sum(len(old[n][1]) for n, _, _ in same)
    lines.append(f'Instructions compared in the identical kernels: {n_ins}.')
    ren = [(n, m) for n, m, _ in same + differ if n != m]
    for title, rows in (('Different', [f'`{n}`: {w}' for n, _, w in differ]), ('Removed', [f'`{n}`' for n in removed]),
                        ('Added', [f'`{n}`' for n in added]),
                        ('Renamed (old -> new)', [f'`{n}` -> `{m}`' for n, m in ren])):
        if rows:
            lines += ['', f'### {title}', ''] + [f'- {r}' for r in rows]
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.md:
        with open(a.md, 'w') as f:
            f.write(text)
    return 1 if differ or added else 0


if __name__ == '__main__':
    sys.exit(main())

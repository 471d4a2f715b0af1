"""Instruction mix of the epilogues of one conv_mm instance in a hipcc -S --offload-device-only listing:
  python tools/diag/epilogue_mix.py <file.s> <mangled-name substring> [--max-valu-per-store X]
An epilogue = the text between two consecutive matrix loops (backward branches whose body holds v_mfma), or between the last matrix loop
and the end of the unit loop around them, that holds at least one global_store_dword; where the next unit's LDS-DMA copy is issued in
between, the text behind it.  Per epilogue: vector-ALU instructions per global_store
(= per stored element: the stores are dwords), and the instructions an epilogue should not need -- 64-bit vector address adds
(v_lshl_add_u64), selects (v_cndmask: one per element is the ReLU mask of a MASKED instance, none otherwise), v_readlane (scalars that
were spilled to vector lanes).  With --max-valu-per-store the exit status says whether every epilogue stays within the bound and is free
of v_lshl_add_u64 / v_readlane.  The same kind of tool as isa_loops.py."""
import re, sys, collections

args = [a for a in sys.argv[1:] if not a.startswith('--')]
bound = float(sys.argv[sys.argv.index('--max-valu-per-store') + 1]) if '--max-valu-per-store' in sys.argv else None
if bound is not None:
    args.remove(sys.argv[sys.argv.index('--max-valu-per-store') + 1])
L = open(args[0]).read().split('\n')
start = next(i for i, l in enumerate(L) if l.startswith('_ZN') and args[1] in l and ':' in l)
end = next(i for i in range(start, len(L)) if L[i].strip().startswith('s_endpgm'))
L = L[start:end + 1]


def ops(a, b):
    return [l.split()[0] for l in L[a:b + 1] if l.startswith('\t') and not l.strip().startswith(('.', ';'))]


lab = {}
for i, l in enumerate(L):
    m = re.match(r'^(\.LBB\d+_\d+):', l)
    if m: lab[m.group(1)] = i
loops = set()
for i, l in enumerate(L):
    m = re.search(r's_c?branch\w*\s+(\.LBB\d+_\d+)', l)
    if m and m.group(1) in lab and lab[m.group(1)] < i:
        loops.add((lab[m.group(1)], i))
has_mfma = lambda a, b: any(o.startswith('v_mfma') for o in ops(a, b))
mm = [lp for lp in loops if has_mfma(*lp)]
# matrix loops = the innermost loops with matrix instructions
inner = sorted(lp for lp in mm if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] for o in mm))
# the unit loop = the outermost loop around all of them (its blocks may be laid out behind an inner backward branch: take the last
# branch back to a label in front of the first matrix loop)
unit_end = max([lp[1] for lp in loops if lp[0] <= inner[0][0] and lp[1] >= inner[-1][1]] or [len(L) - 1])
print('%d lines, %d matrix loops, unit loop ends at line %d' % (len(L), len(inner), unit_end))
regions = [(inner[k][1] + 1, (inner[k + 1][0] if k + 1 < len(inner) else unit_end) - 1) for k in range(len(inner))]
bad = False
nep = 0
is_store = lambda l: l.split()[:1] == ['global_store_dword']            # (the statistics flush stores dwordx4: not an element)
for a, b in regions:
    first = next((i for i in range(a, b + 1) if is_store(L[i])), None)
    if first is None: continue
    # the next unit's copy (single-buffered instances issue it ahead of the stores) and its barrier are not the epilogue
    a = max([a] + [i + 1 for i in range(a, first) if L[i].split()[:1] and L[i].split()[0] in ('s_barrier', 'global_load_lds_dwordx4', 'global_load_lds_dword')])
    c = collections.Counter(ops(a, b))
    st = c['global_store_dword']
    nep += 1
    valu = sum(v for k, v in c.items() if k.startswith('v_') and not k.startswith('v_mfma'))
    salu = sum(v for k, v in c.items() if k.startswith('s_') and k not in ('s_waitcnt', 's_nop'))
    pk = sum(v for k, v in c.items() if k.startswith('v_pk_'))
    saddr = sum(1 for l in L[a:b + 1] if is_store(l) and re.search(r',\s*s\[\d+:\d+\]', l))
    print('lines %5d-%5d: stores %3d (scalar base %3d)  valu %4d = %.2f per store  (packed %d)  salu %4d  v_cndmask %3d  v_lshl_add_u64 %3d  '
          'v_readlane %3d  v_mov %3d  global_load %3d' % (a, b, st, saddr, valu, valu / st, pk, salu, c['v_cndmask_b32'] + c['v_cndmask_b32_e32'] + c['v_cndmask_b32_e64'],
                                                        c['v_lshl_add_u64'], c['v_readlane_b32'], sum(v for k, v in c.items() if k.startswith('v_mov')),
                                                        sum(v for k, v in c.items() if k.startswith('global_load'))))
    if bound is not None and (valu / st > bound or c['v_lshl_add_u64'] or c['v_readlane_b32']): bad = True
if not nep: print('no epilogue found'); bad = True
sys.exit(1 if bad else 0)

"""Per kernel name: launches and time per step of the style-path rows (same 16-step window as step_breakdown.py)."""
import csv
import sys
from collections import defaultdict

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r['Start_Timestamp']))
ms = float(sys.argv[2])
c64 = [r for r in rows if 'conv3x3_c64r' in r['Kernel_Name']] or [r for r in rows if 'conv3x3_c64p' in r['Kernel_Name']]
halo = [r for r in rows if 'conv3x3_halo' in r['Kernel_Name']]
if len(c64) > 23:
    t_end = int(c64[-23]['Start_Timestamp'])
else:
    t_end = int(halo[-23 - 23]['Start_Timestamp']) if len(halo) > 46 else int(halo[0]['Start_Timestamp'])
t0 = t_end - int(16 * ms * 1e6)
agg = defaultdict(lambda: [0, 0])
for r in rows:
    n = r['Kernel_Name']
    if t0 <= int(r['Start_Timestamp']) < t_end and any(k in n for k in ('demod', 'infnorm', 'pack_weight', 'style_table', 'split3')):
        a = agg[n[:100]]
        a[0] += int(r['End_Timestamp']) - int(r['Start_Timestamp'])
        a[1] += 1
tt = tn = 0
for k, (t, n) in sorted(agg.items(), key=lambda kv: -kv[1][0]):
    print(f'{t / 16e6:7.3f} ms/step {n / 16:7.1f} launches/step  {k}')
    tt += t
    tn += n
print(f'{tt / 16e6:7.3f} ms/step {tn / 16:7.1f} launches/step  sum of the style-path rows (demod, pre-normalisation, weight pack, f32 split, style table)')

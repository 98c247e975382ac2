"""Per-kernel times of the batched adjoint against the single-member one, from rocprofv3 kernel summaries.

    for b in 2 4 8 16; do
        rocprofv3 --kernel-trace --stats --output-format csv -d prof/b$b -- \\
            python profiles/microbench/grad_batch_bw.py --cases 100k_month_b$b --reps 1 --warmup 1
    done
    python profiles/microbench/grad_batch_kernel_stats.py prof profiles/grad_batch_kernel_stats.csv

Each run is one process with one case: the loop of B single-member calls (the kernels without a member dimension) and one batched
call (`ENS = true`, `*_batch`), twice (a warm-up and one repetition, both in the summary).  rocprofv3 sums by kernel name, so the
member counts need a run each; this script puts the engine's kernels of every run into one table with the member count in front.
MedianStartToStartNs comes from the trace itself: the median time from the start of one dispatch of a kernel to the start of its
next, over pairs less than 1 ms apart (the ticks of one sweep).  Where it exceeds the kernel's own time the sweep waits on launches."""
import csv
import glob
import os
import re
import sys


def name_of(full):
    return re.sub(r'^void ', '', full.replace('(anonymous namespace)::', '')).split('(')[0]


def intervals(d):
    """median start-to-start time of consecutive dispatches of each kernel, or {} without a trace file"""
    found = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    if len(found) != 1:
        return {}
    starts = {}
    with open(found[0], newline='') as f:
        for r in csv.DictReader(f):
            starts.setdefault(name_of(r['Kernel_Name']), []).append(int(r['Start_Timestamp']))
    out = {}
    for name, t in starts.items():
        t.sort()
        gaps = sorted(b - a for a, b in zip(t, t[1:]) if b - a < 1_000_000)
        if gaps:
            out[name] = gaps[len(gaps) // 2]
    return out


def main(src, dst):
    rows = []
    for d in sorted(glob.glob(os.path.join(src, 'b*')), key=lambda p: int(os.path.basename(p)[1:])):
        gap = intervals(d)
        (stats,) = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        with open(stats, newline='') as f:
            for r in csv.DictReader(f):
                name = name_of(r['Name'])
                if not re.match(r'k_(tick|adj_|perm_)', name):
                    continue
                rows.append([int(os.path.basename(d)[1:]), name, int(r['Calls']), int(r['TotalDurationNs']), float(r['AverageNs']),
                             int(r['MinNs']), int(r['MaxNs']), float(r['StdDev']), gap.get(name, '')])
    with open(dst, 'w', newline='') as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(['Members', 'Name', 'Calls', 'TotalDurationNs', 'AverageNs', 'MinNs', 'MaxNs', 'StdDev', 'MedianStartToStartNs'])
        w.writerows(rows)


if __name__ == '__main__':
    main(*sys.argv[1:3])

"""Per-layer kernel durations of ConvNetwork.test_sequence_any from rocprofv3 kernel traces:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python experiments/seq_any_timing.py --child any --batches B
    python experiments/seq_any_kernel_times.py DIR [DIR ...]

The launches of k_lif_seq_any are grouped by (template instance, LDS bytes, grid): one group per layer of the network (layers that
share an instance differ in their LDS size); per group the number of launches, the median and the fastest duration.  The other
kernels of the sequence (k_seq_any_wprep, k_pack_planes, readouts, votes) are listed by name."""
import collections
import csv
import os
import statistics
import sys


def key_like(row, *parts):
    for k in row:
        if all(p.lower() in k.lower() for p in parts):
            return k
    return None


def main():
    for d in sys.argv[1:]:
        files = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_trace.csv")]
        groups = collections.defaultdict(list)
        for path in files:
            with open(path, newline="") as f:
                rd = csv.DictReader(f)
                for row in rd:
                    kn, ks, ke = key_like(row, "kernel_name"), key_like(row, "start"), key_like(row, "end")
                    kl, kg = key_like(row, "lds"), key_like(row, "grid_size") or key_like(row, "grid")
                    name = row[kn].split("(")[0]
                    if "k_lif_seq_any" in name:
                        k = (name, row.get(kl, "?"), row.get(kg, "?"))
                    else:
                        k = (name, "", "")
                    groups[k].append((int(row[ke]) - int(row[ks])) / 1e3)
        print("%s: %d trace file(s)" % (d, len(files)))
        for k, v in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
            if "seq_any" in k[0] or "pack_planes" in k[0] or "readout" in k[0] or "vote" in k[0] or "argmax" in k[0]:
                print("  %-60s lds %8s grid %8s  n %4d  median %9.1f us  min %9.1f us  total %9.1f us"
                      % (k[0][-60:], k[1], k[2], len(v), statistics.median(v), min(v), sum(v)))
        print()


if __name__ == "__main__":
    main()

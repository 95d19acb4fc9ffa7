#!/usr/bin/env python
"""Caption consistency per object from a CSV of captions - the computation of the reference's scripts/compute_cosine_sim.py (not
its plots): rows `episode_id, object_id, caption` are grouped by (episode_id, object_id), every caption is embedded with the
sentence encoder and each group's MEAN PAIRWISE COSINE over its captions (i < j, repeats included) is written next to the overall
mean of the groups that have a pair.

    python tools/caption_consistency_csv.py captions.csv --out consistency.csv [--model all-MiniLM-L6-v2] [--device cuda:0]

Output CSV: `episode_id, object_id, captions, pairs, mean_cosine, std_cosine, disagreement, medoid_caption`, one row per group in
first-seen order, then a last row `overall, , <groups with a pair>, , <mean of their mean_cosine>, , ,`.  Distinct captions are
embedded once and counted (similarity.group_similarity's weights): a group of one caption, or of n copies of one caption, has
pairs = n (n - 1) / 2 and, with no pair, takes no part in the overall mean."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_groups(path):
    """-> {(episode_id, object_id): [caption, ...]} in first-seen order; a header row naming the three columns is skipped"""
    grouped = {}
    with open(path, newline="") as f:
        for i, row in enumerate(csv.reader(f)):
            if not row or len(row) < 3:
                continue
            ep, ob, cap = row[0].strip(), row[1].strip(), row[2]
            if i == 0 and ep.lower() in ("episode_id", "episode") and "caption" in cap.lower():
                continue
            grouped.setdefault((ep, ob), []).append(cap)
    return grouped


def consistency(grouped, encoder):
    """-> (rows, overall): rows = [(episode_id, object_id, captions, pairs, mean, std, disagreement, medoid_caption)], overall = the
    mean of `mean` over the groups with at least one pair (None when there is none)"""
    from embodied_captioning_amd.distributed import captions_frequency
    stats = encoder.caption_statistics(captions_frequency(grouped))
    rows = [(k[0], k[1], len(grouped[k]), s["pairs"], s["mean"], s["std"], s["disagreement"], s["medoid_caption"]) for k, s in stats.items()]
    with_pairs = [r[4] for r in rows if r[3] > 0]
    return rows, (sum(with_pairs) / len(with_pairs) if with_pairs else None)


def write_csv(path, rows, overall):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["episode_id", "object_id", "captions", "pairs", "mean_cosine", "std_cosine", "disagreement", "medoid_caption"])
        w.writerows(rows)
        w.writerow(["overall", "", sum(1 for r in rows if r[3] > 0), "", "" if overall is None else overall, "", "", ""])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("csv", help="episode_id, object_id, caption")
    ap.add_argument("--out", required=True)
    ap.add_argument("--model", default="all-MiniLM-L6-v2")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--batch_size", type=int, default=64)
    a = ap.parse_args(argv)
    from embodied_captioning_amd.captioner.sentence_encoder import SentenceEncoder
    rows, overall = consistency(read_groups(a.csv), SentenceEncoder(a.model, device=a.device, dtype="f32", batch_size=a.batch_size))
    write_csv(a.out, rows, overall)
    print(f"{len(rows)} groups, overall mean pairwise cosine {overall}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""Turn a results folder into a pseudo-label annotation file: the detections of ``bbox.json`` / ``segm.json`` -- the files
``tools/infer_net.py --export-results`` writes -- above a score threshold become the annotations of a COCO-format file whose
masks are the results' compressed RLEs.  The dataset reader trains from it (data/datasets.py: ``RleMasks``), so a teacher's
confident detections on a captioned set can train a student offline.  Host only: nothing is decoded here.

  python tools/results_to_annotations.py --ann-file instances.json --results-dir OUTPUT_DIR/inference/<name> \\
      --score-threshold 0.8 --output pseudo_instances.json

The exporter writes both files in the same order, so entry k of one is entry k of the other: ``image_id``, ``category_id``
and ``score`` must agree for every pair.  The output keeps the annotation file's ``images`` and ``categories`` as they are
(embeddings and splits included); each kept pair becomes {id, image_id, category_id, bbox, segmentation: {size, counts},
area, iscrowd: 0, score}, ids counted from 1 in file order.
"""
import argparse
import json
import os
import sys


def convert(dataset, boxes, masks, score_threshold):
    """-> the pseudo-label dataset dict.  Raises ValueError naming the first index at which the two lists disagree."""
    if len(boxes) != len(masks):
        raise ValueError(f"bbox.json has {len(boxes)} entries, segm.json {len(masks)}: they are not one export")
    known = {img["id"] for img in dataset["images"]}
    annotations = []
    for k, (b, m) in enumerate(zip(boxes, masks)):
        for key in ("image_id", "category_id", "score"):
            if b.get(key) != m.get(key):
                raise ValueError(f"entry {k}: bbox.json has {key} {b.get(key)!r}, segm.json {m.get(key)!r}: the files are "
                                 "paired by position and must come from one export")
        if b["image_id"] not in known:
            raise ValueError(f"entry {k}: image_id {b['image_id']!r} is not an image of the annotation file")
        seg = m.get("segmentation")
        if not isinstance(seg, dict) or "size" not in seg or "counts" not in seg:
            raise ValueError(f"entry {k}: segm.json has no RLE segmentation {{size, counts}}")
        if b["score"] < score_threshold:
            continue
        box = [float(v) for v in b["bbox"]]
        annotations.append({"id": len(annotations) + 1, "image_id": b["image_id"], "category_id": b["category_id"], "bbox": box,
                            "segmentation": {"size": [int(v) for v in seg["size"]], "counts": seg["counts"]},
                            "area": box[2] * box[3], "iscrowd": 0, "score": b["score"]})
    out = {k: v for k, v in dataset.items() if k != "annotations"}
    out["annotations"] = annotations
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(description="bbox.json + segm.json above a score threshold -> a COCO annotation file "
                                                 "with RLE masks")
    parser.add_argument("--ann-file", required=True, metavar="FILE", help="the annotation file the results were made on")
    parser.add_argument("--results-dir", required=True, metavar="DIR", help="holds bbox.json and segm.json of one export")
    parser.add_argument("--score-threshold", type=float, default=0.5, help="keep detections with score >= this")
    parser.add_argument("--output", required=True, metavar="PATH", help="the annotation file to write")
    args = parser.parse_args(argv)
    paths = {name: os.path.join(args.results_dir, name + ".json") for name in ("bbox", "segm")}
    for path in [args.ann_file] + list(paths.values()):
        if not os.path.exists(path):
            parser.error(f"{path} does not exist")
    loaded = {}
    for name, path in dict(paths, ann=args.ann_file).items():
        with open(path) as f:
            loaded[name] = json.load(f)
    try:
        out = convert(loaded["ann"], loaded["bbox"], loaded["segm"], args.score_threshold)
    except ValueError as e:
        sys.exit(f"results_to_annotations: {e}")
    with open(args.output, "w") as f:
        json.dump(out, f)
    print(f"{len(out['annotations'])} of {len(loaded['bbox'])} detections kept (score >= {args.score_threshold}) -> {args.output}")
    return out


if __name__ == "__main__":
    main()

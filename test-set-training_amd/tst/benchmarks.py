"""Benchmark adapters ("benchmark loaders (VSI-Bench / CV-Bench / MMMU / VideoMME text-only)"; the reference README names
these four and ships VSI-Bench-Debiased): rows of a LOCAL copy of a benchmark's published table -> the text-only QA records the fold loop
reads ({"id", "question", "options", "answer", "src_id", "group"}; tst.io.load_qa_jsonl). Images and videos are never touched: the diagnostic
is text-only by construction (README.md:35). Nothing is downloaded here -- `path` is a parquet / JSON / JSONL / CSV file the user already has.

Column names follow the dataset cards (nyu-visionx/VSI-Bench, nyu-visionx/CV-Bench, MMMU/MMMU, lmms-lab/Video-MME). They could not be checked
against the real files offline; every adapter fails with the list of columns it found when a required one is missing, and `columns=` remaps
names for a differently exported copy.

Row order defines the integer `id` the fold loop, the score records and the debiased export are keyed by; `src_id` keeps the benchmark's own
identifier, and `filter_table` writes the surviving ROWS of the original table (all columns, original order) -- what VSI-Bench-Debiased is to
VSI-Bench."""
import ast
import csv
import json
import re

LETTERS = "ABCDEFGH"
_PREFIX = re.compile(r"^\s*\(?([A-H])[\).:]\s*")


def read_table(path):
    """list of row dicts from .parquet (pyarrow), .json (list or {"data": [...]}), .jsonl or .csv"""
    p = str(path).lower()
    if p.endswith(".parquet"):
        import pyarrow.parquet as pq
        return pq.read_table(path).to_pylist()
    if p.endswith(".jsonl"):
        with open(path) as f:
            return [json.loads(line) for line in f if line.strip()]
    if p.endswith(".json"):
        with open(path) as f:
            d = json.load(f)
        return d["data"] if isinstance(d, dict) and "data" in d else d
    if p.endswith(".csv"):
        with open(path, newline="") as f:
            return list(csv.DictReader(f))
    raise ValueError(f"{path}: unknown table format (parquet, json, jsonl, csv)")


def _options(raw):
    """a benchmark's option field -> list of option texts without their letter prefix ("A. sofa", "(B) chair" -> "sofa", "chair")"""
    if raw is None:
        return []
    if isinstance(raw, str):
        t = raw.strip()
        if not t:
            return []
        if t[0] in "[(":                      # MMMU stores the python repr of a list
            raw = ast.literal_eval(t)
        else:
            raw = [x for x in t.split("\n") if x.strip()]
    out = []
    for i, o in enumerate(list(raw)):
        o = str(o)
        m = _PREFIX.match(o)
        out.append(o[m.end():] if m and m.group(1) == LETTERS[min(i, 7)] else o.strip())
    return out


def _letter(ans):
    """"B", "(B)", "B." -> "B"; anything else -> None"""
    m = re.fullmatch(r"\s*\(?([A-Ha-h])[\).]?\s*", str(ans))
    return m.group(1).upper() if m else None


def _need(row, cols, names, what):
    miss = [cols.get(n, n) for n in names if cols.get(n, n) not in row]
    if miss:
        raise KeyError(f"{what}: missing column(s) {miss}; the table has {sorted(row)} (pass columns={{...}} to remap)")


def _record(i, question, options, answer, src_id, group):
    options = [o for o in options if o != ""]
    if options:
        L = _letter(answer)
        if L is None:                         # the answer is the option TEXT (some exports do that): map it back to its letter
            hits = [j for j, o in enumerate(options) if o.strip().lower() == str(answer).strip().lower()]
            if len(hits) != 1:
                raise ValueError(f"row {i} ({src_id}): answer {answer!r} is neither an option letter nor exactly one of the options")
            L = LETTERS[hits[0]]
        if LETTERS.index(L) >= len(options):
            raise ValueError(f"row {i} ({src_id}): answer {L} beyond the {len(options)} options")
        answer = L
    return dict(id=i, question=str(question).strip(), options=options, answer=str(answer).strip(), src_id=src_id, group=group)


def from_vsi_bench(rows, columns=None):
    """nyu-visionx/VSI-Bench: id, dataset, scene_name, question_type, question, options (list of "A. ..." or null), ground_truth (option letter
    for the multiple-choice types, a number for object_counting / *_distance / *_size_estimation)"""
    c = columns or {}
    out = []
    for i, r in enumerate(rows):
        _need(r, c, ("question", "ground_truth"), "VSI-Bench")
        out.append(_record(i, r[c.get("question", "question")], _options(r.get(c.get("options", "options"))), r[c.get("ground_truth", "ground_truth")],
                           r.get(c.get("id", "id"), i), r.get(c.get("question_type", "question_type"))))
    return out


def from_cv_bench(rows, columns=None):
    """nyu-visionx/CV-Bench: idx, type (2D / 3D), task (Count, Relation, Depth, Distance), question, choices (list), answer ("(C)")"""
    c = columns or {}
    out = []
    for i, r in enumerate(rows):
        _need(r, c, ("question", "choices", "answer"), "CV-Bench")
        out.append(_record(i, r[c.get("question", "question")], _options(r[c.get("choices", "choices")]), r[c.get("answer", "answer")],
                           r.get(c.get("idx", "idx"), i), r.get(c.get("task", "task"))))
    return out


def from_mmmu(rows, columns=None):
    """MMMU/MMMU: id ("validation_Accounting_1"), question (with <image 1> markers, kept as text), options (python-list string), answer (letter, or
    free text for question_type "open"), question_type"""
    c = columns or {}
    out = []
    for i, r in enumerate(rows):
        _need(r, c, ("question", "answer"), "MMMU")
        out.append(_record(i, r[c.get("question", "question")], _options(r.get(c.get("options", "options"))), r[c.get("answer", "answer")],
                           r.get(c.get("id", "id"), i), r.get(c.get("question_type", "question_type"))))
    return out


def from_videomme(rows, columns=None):
    """lmms-lab/Video-MME: video_id, duration, domain, sub_category, question_id, task_type, question, options (["A. ...", ...]), answer (letter)"""
    c = columns or {}
    out = []
    for i, r in enumerate(rows):
        _need(r, c, ("question", "options", "answer"), "Video-MME")
        out.append(_record(i, r[c.get("question", "question")], _options(r[c.get("options", "options")]), r[c.get("answer", "answer")],
                           r.get(c.get("question_id", "question_id"), i), r.get(c.get("task_type", "task_type"))))
    return out


ADAPTERS = {"vsi-bench": from_vsi_bench, "cv-bench": from_cv_bench, "mmmu": from_mmmu, "videomme": from_videomme}


def convert(benchmark, src, dst_jsonl, columns=None):
    """local benchmark table -> QA JSONL for `tst.cli diagnose / prune / rf --data-file`; returns (n, n_multiple_choice)"""
    if benchmark not in ADAPTERS:
        raise ValueError(f"unknown benchmark {benchmark!r} ({', '.join(ADAPTERS)})")
    recs = ADAPTERS[benchmark](read_table(src), columns)
    with open(dst_jsonl, "w") as f:
        for r in recs:
            f.write(json.dumps(r, ensure_ascii=False) + "\n")
    return len(recs), sum(1 for r in recs if r["options"])


def filter_table(src, dst, keep_ids):
    """the debiased benchmark as a table: the rows of `src` whose ROW INDEX (= the id `convert` assigned) survived, every column kept, original
    order; parquet -> parquet (schema preserved), otherwise JSONL. Returns (kept, dropped)."""
    keep = set(int(i) for i in keep_ids)
    if str(src).lower().endswith(".parquet"):
        import pyarrow.parquet as pq
        t = pq.read_table(src)
        idx = [i for i in range(t.num_rows) if i in keep]
        out = t.take(idx)
        if str(dst).lower().endswith(".parquet"):
            pq.write_table(out, dst)
        else:
            with open(dst, "w") as f:
                for r in out.to_pylist():
                    f.write(json.dumps(r, ensure_ascii=False, default=str) + "\n")
        return len(idx), t.num_rows - len(idx)
    rows = read_table(src)
    kept = [r for i, r in enumerate(rows) if i in keep]
    with open(dst, "w") as f:
        for r in kept:
            f.write(json.dumps(r, ensure_ascii=False, default=str) + "\n")
    return len(kept), len(rows) - len(kept)


# ---- VSI-Bench's metric for numeric answers
_NUMBER = re.compile(r"[-+]?(?:\d+(?:\.\d*)?|\.\d+)(?:[eE][-+]?\d+)?")


def parse_number(text):
    """the first number in a decoded answer ("about 2.5 m" -> 2.5, " 3" -> 3.0; thousands separators are not read: "1,200" -> 1.0), or None"""
    if isinstance(text, (int, float)) and not isinstance(text, bool):
        return float(text) if text == text and abs(text) != float("inf") else None
    m = _NUMBER.search(str(text))
    if m is None:
        return None
    try:
        v = float(m.group(0))
    except ValueError:
        return None
    return v if abs(v) != float("inf") else None


def mean_relative_accuracy(pred, ref):
    """VSI-Bench's mean relative accuracy of one prediction: the mean over theta in {0.50, 0.55, ..., 0.95} of 1[|pred - ref| / |ref| < 1 - theta]. pred / ref:
    numbers or text (parse_number); an unparseable prediction scores 0, an unparseable reference raises ValueError. The comparison is exact in the decimal
    values as written (0.9 against 1 has relative error exactly 0.1, which is not < 0.1). ref = 0 has no relative error: 1 if pred == 0, else 0."""
    from fractions import Fraction
    r = parse_number(ref)
    if r is None:
        raise ValueError(f"reference answer is not a number: {ref!r}")
    p = parse_number(pred)
    if p is None:
        return 0.0
    p, r = Fraction(repr(p)), Fraction(repr(r))
    if r == 0:
        return 1.0 if p == 0 else 0.0
    rel = abs(p - r) / abs(r)
    return sum(1 for k in range(10) if rel < Fraction(50 - 5 * k, 100)) / 10.0

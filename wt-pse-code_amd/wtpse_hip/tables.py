"""The tables the run programs write: one CSV form and one JSON form.  A CSV holds a header and one line per row; the column called
"name" is quoted when it holds a comma, a quote or a newline, the other text columns are written as they are, an int column as
str(int(v)) and every other column as repr(float(v)) — it reads back to the same float64, nan as "nan"."""
import csv
import json


def _quoted(name):
    name = str(name)
    return '"' + name.replace('"', '""') + '"' if any(ch in name for ch in ',"\n') else name


def write_csv(path, columns, rows, ints=(), texts=("name",)):
    with open(path, "w") as f:
        f.write(",".join(columns) + "\n")
        for r in rows:
            f.write(",".join(_quoted(r[k]) if k == "name" else str(r[k]) if k in texts else str(int(r[k])) if k in ints else repr(float(r[k]))
                             for k in columns) + "\n")


def read_csv(path, ints=(), texts=("name",)):
    """-> the rows as write_csv wrote them: the file's columns in its order, str / int / float by the same two sets."""
    with open(path, newline="") as f:
        return [{k: v if k in texts else int(v) if k in ints else float(v) for k, v in r.items()} for r in csv.DictReader(f)]


def write_json(path, obj, allow_nan):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True, allow_nan=allow_nan)
        f.write("\n")


def read_json(path):
    with open(path) as f:
        return json.load(f)

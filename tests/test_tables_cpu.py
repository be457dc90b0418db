"""The run programs' tables: every public writer's bytes against literals recorded from the writers as they stood before they shared
wtpse_hip.tables (rows with nan, inf, a name holding a comma and a quote, int columns given as numpy integers and floats given as
ints), and the shared pair's own round trip."""
import math
import os

import numpy as np
import pytest

NAMES = ("a.png", 'he said "x", ok.png', "plain name.png")
TEXTS = ("disc", "cup", "left")
NAN = float("nan")


def rows_for(columns, ints, texts=("name",)):
    """Three rows over `columns`: ints as 3 + 7 i + j (row 1 as numpy integers), floats from a small cycle that holds nan, inf, an
    integer-valued float and a Python int."""
    rows = []
    for i in range(3):
        row = {}
        for j, k in enumerate(columns):
            if k == "name":
                row[k] = NAMES[i]
            elif k in texts:
                row[k] = TEXTS[i]
            elif k in ints:
                row[k] = np.int64(3 + 7 * i + j) if i == 1 else 3 + 7 * i + j
            else:
                row[k] = (0.1 * (i + 1) + j / 3.0, NAN, -2.0, float("inf"), 7, 1e-7 * (j + 1))[(i + j) % 6]
        rows.append(row)
    return rows


def _written(tmp_path, write):
    out = tmp_path / "out"
    out.mkdir()
    write(str(out))
    got = {}
    for f in sorted(os.listdir(out)):
        with open(out / f, newline="") as fh:
            got[f] = fh.read()
    return got


def _segment(out):
    from wtpse_hip import segment as S
    S.write_measurements(out, rows_for(S.CSV_COLUMNS, ("index",) + S.INT_COLUMNS), {"n": 3, "mean_vcdr": None, "mean_hcdr": 0.25})


def _test_run(out):
    from wtpse_hip import test_run as T
    T.write_table(out, rows_for(T.CSV_COLUMNS, ("index",)), {"n": 3, "disc_dice": NAN, "cup_dice": 0.5})


def _uncertainty(out):
    from wtpse_hip import uncertainty as U
    U.write_csv(out, rows_for(U.CSV_COLUMNS, ("index", "n_samples", "n_defined", "disc_disagree_px", "cup_disagree_px")))


def _calibration(out):
    from wtpse_hip import calibration as C
    for table, (columns, ints, texts) in C.TABLES.items():
        C.write_csv(out, table, rows_for(columns, ints, texts))
    C.write_summary(out, {"n": 3, "scales": [0.0, 0.5], "disc": {"lowest_nll": None}})


def _morph_rows():
    from wtpse_hip import morphometry as M
    rows = rows_for(M.MORPH_COLUMNS, ("index",) + M.INT_COLUMNS, ("name", "eye"))
    for i, r in enumerate(rows):
        r.update(sectors=8, rim=[NAN if s == i else s + 0.5 * i for s in range(8)], eye=(None, "right", "left")[i])
    return rows


def _morphometry(out):
    from wtpse_hip import morphometry as M
    M.write_csv(out, _morph_rows())
    unc = rows_for(("index", "name") + M.STAT_COLUMNS, ("index", "n_samples", "n_defined"))
    for i, r in enumerate(unc):
        r["rim_rel_std"] = [NAN if s == i else 0.125 * s + i for s in range(8)]
    M.write_uncertainty_csv(out, unc)
    M.write_errors_csv(out, rows_for(("index", "name") + M.ERROR_COLUMNS, ("index",))[:2])


def _locate(out):
    from wtpse_hip import locate as L
    L.write_roi_csv(out, rows_for(L.ROI_COLUMNS, ("index",) + L._INTS))


WRITERS = {"segment": _segment, "test_run": _test_run, "uncertainty": _uncertainty, "calibration": _calibration,
           "morphometry": _morphometry, "locate": _locate}

# recorded once from the writers of the commit before wtpse_hip.tables existed, on exactly the rows above
EXPECTED = {
    'calibration': {
        'calibration.csv': (
            'scale,structure,n_scored,n_excluded_neg,n_excluded_pos,n_invalid,ece,mce,brier,nll,auroc,error_rate,spread_wrong_mean,spread_right_mean,spread_auroc,vcdr_coverage,hcdr_coverage,acdr_coverage,vcdr_spearman,n_defined\n'
            '0.1,disc,5,6,7,8,2.1,nan,-2.0,inf,7.0,1.2e-06,4.1,nan,-2.0,inf,7.0,1.8e-06,6.1,22\n'
            'nan,cup,12,13,14,15,nan,-2.0,inf,7.0,1.1e-06,3.8666666666666667,nan,-2.0,inf,7.0,1.6999999999999998e-06,5.866666666666667,nan,29\n'
            '-2.0,left,19,20,21,22,-2.0,inf,7.0,1e-06,3.6333333333333337,nan,-2.0,inf,7.0,1.6e-06,5.633333333333333,nan,-2.0,36\n'
        ),
        'per_image.csv': (
            'scale,index,name,disc_dice,cup_dice,vcdr_label,vcdr_pred,vcdr_mean,vcdr_std,vcdr_p05,vcdr_p95,hcdr_label,hcdr_pred,hcdr_mean,hcdr_std,hcdr_p05,hcdr_p95,acdr_label,acdr_pred,acdr_mean,acdr_std,acdr_p05,acdr_p95,vcdr_inside,disc_ece,cup_ece\n'
            '0.1,4,a.png,inf,7.0,6e-07,2.1,nan,-2.0,inf,7.0,1.2e-06,4.1,nan,-2.0,inf,7.0,1.8e-06,6.1,nan,-2.0,inf,7.0,2.4e-06,8.1,nan\n'
            'nan,11,"he said ""x"", ok.png",7.0,5e-07,1.8666666666666667,nan,-2.0,inf,7.0,1.1e-06,3.8666666666666667,nan,-2.0,inf,7.0,1.6999999999999998e-06,5.866666666666667,nan,-2.0,inf,7.0,2.3e-06,7.866666666666667,nan,-2.0\n'
            '-2.0,18,plain name.png,4e-07,1.6333333333333333,nan,-2.0,inf,7.0,1e-06,3.6333333333333337,nan,-2.0,inf,7.0,1.6e-06,5.633333333333333,nan,-2.0,inf,7.0,2.2e-06,7.633333333333333,nan,-2.0,inf\n'
        ),
        'reliability.csv': (
            'scale,structure,bin,lo,hi,n,mean_conf,frac_pos\n'
            '0.1,disc,5,inf,7.0,8,2.1,nan\n'
            'nan,cup,12,7.0,5e-07,15,nan,-2.0\n'
            '-2.0,left,19,4e-07,1.6333333333333333,22,-2.0,inf\n'
        ),
        'risk_coverage.csv': (
            'scale,structure,level,coverage,risk\n'
            '0.1,disc,disc,inf,7.0\n'
            'nan,cup,cup,7.0,5e-07\n'
            '-2.0,left,left,4e-07,1.6333333333333333\n'
        ),
        'summary.json': (
            '{\n'
            ' "disc": {\n'
            '  "lowest_nll": null\n'
            ' },\n'
            ' "n": 3,\n'
            ' "scales": [\n'
            '  0.0,\n'
            '  0.5\n'
            ' ]\n'
            '}\n'
        ),
    },
    'locate': {
        'roi.csv': (
            'index,name,height,width,fov_area,fov_diameter,cell,window,located,verified,candidate,score,roi_top,roi_left,roi_side,refine_rounds,disc_cy,disc_cx,cup_cy,cup_cx\n'
            '3,a.png,5,6,7,6e-07,9,10,11,12,13,1.2e-06,15,16,17,18,7.0,1.8e-06,6.1,nan\n'
            '10,"he said ""x"", ok.png",12,13,14,1.8666666666666667,16,17,18,19,20,3.8666666666666667,22,23,24,25,1.6999999999999998e-06,5.866666666666667,nan,-2.0\n'
            '17,plain name.png,19,20,21,nan,23,24,25,26,27,nan,29,30,31,32,5.633333333333333,nan,-2.0,inf\n'
        ),
    },
    'morphometry': {
        'morphometry.csv': (
            'index,name,eye,height,width,sectors,disc_area,cup_area,centre_y,centre_x,disc_major,disc_minor,disc_angle,disc_v_extent,disc_h_extent,cup_major,cup_minor,cup_angle,cup_v_extent,cup_h_extent,vcdr_ellipse,hcdr_ellipse,rim_min,rim_min_rel,rim_min_angle,rim_superior,rim_inferior,rim_left,rim_right,rim_nasal,rim_temporal,isnt\n'
            '3,a.png,None,6,7,8,9,10,-2.0,inf,7.0,1.2e-06,4.1,nan,-2.0,inf,7.0,1.8e-06,6.1,nan,-2.0,inf,7.0,2.4e-06,8.1,nan,-2.0,inf,7.0,3e-06,10.1,nan\n'
            '10,"he said ""x"", ok.png",right,13,14,8,16,17,inf,7.0,1.1e-06,3.8666666666666667,nan,-2.0,inf,7.0,1.6999999999999998e-06,5.866666666666667,nan,-2.0,inf,7.0,2.3e-06,7.866666666666667,nan,-2.0,inf,7.0,2.8999999999999998e-06,9.866666666666665,nan,-2.0\n'
            '17,plain name.png,left,20,21,8,23,24,7.0,1e-06,3.6333333333333337,nan,-2.0,inf,7.0,1.6e-06,5.633333333333333,nan,-2.0,inf,7.0,2.2e-06,7.633333333333333,nan,-2.0,inf,7.0,2.8e-06,9.633333333333335,nan,-2.0,inf\n'
        ),
        'morphometry_errors.csv': (
            'index,name,vcdr_ellipse_pred,vcdr_ellipse_label,vcdr_ellipse_abs_diff,hcdr_ellipse_pred,hcdr_ellipse_label,hcdr_ellipse_abs_diff,rim_min_rel_pred,rim_min_rel_label,rim_min_rel_abs_diff\n'
            '3,a.png,-2.0,inf,7.0,6e-07,2.1,nan,-2.0,inf,7.0\n'
            '10,"he said ""x"", ok.png",inf,7.0,5e-07,1.8666666666666667,nan,-2.0,inf,7.0,1.1e-06\n'
            '0,mean,inf,inf,3.50000025,0.9333336333333333,2.1,-2.0,inf,inf,3.50000055\n'
        ),
        'morphometry_uncertainty.csv': (
            'index,name,n_samples,n_defined,vcdr_ellipse_mean,vcdr_ellipse_std,vcdr_ellipse_p05,vcdr_ellipse_p95,hcdr_ellipse_mean,hcdr_ellipse_std,hcdr_ellipse_p05,hcdr_ellipse_p95,rim_min_rel_mean,rim_min_rel_std,rim_min_rel_p05,rim_min_rel_p95,rim_rel_std_000,rim_rel_std_001,rim_rel_std_002,rim_rel_std_003,rim_rel_std_004,rim_rel_std_005,rim_rel_std_006,rim_rel_std_007\n'
            '3,a.png,5,6,7.0,6e-07,2.1,nan,-2.0,inf,7.0,1.2e-06,4.1,nan,-2.0,inf,nan,0.125,0.25,0.375,0.5,0.625,0.75,0.875\n'
            '10,"he said ""x"", ok.png",12,13,5e-07,1.8666666666666667,nan,-2.0,inf,7.0,1.1e-06,3.8666666666666667,nan,-2.0,inf,7.0,1.0,nan,1.25,1.375,1.5,1.625,1.75,1.875\n'
            '17,plain name.png,19,20,1.6333333333333333,nan,-2.0,inf,7.0,1e-06,3.6333333333333337,nan,-2.0,inf,7.0,1.6e-06,2.0,2.125,nan,2.375,2.5,2.625,2.75,2.875\n'
        ),
        'rim_profile.csv': (
            'index,name,rim_000,rim_001,rim_002,rim_003,rim_004,rim_005,rim_006,rim_007\n'
            '3,a.png,nan,1.0,2.0,3.0,4.0,5.0,6.0,7.0\n'
            '10,"he said ""x"", ok.png",0.5,nan,2.5,3.5,4.5,5.5,6.5,7.5\n'
            '17,plain name.png,1.0,2.0,nan,4.0,5.0,6.0,7.0,8.0\n'
        ),
    },
    'segment': {
        'measurements.csv': (
            'index,name,height,width,disc_area,cup_area,disc_top,disc_bottom,disc_left,disc_right,cup_top,cup_bottom,cup_left,cup_right,disc_cy,disc_cx,cup_cy,cup_cx,vcdr,hcdr,acdr\n'
            '3,a.png,5,6,7,8,9,10,11,12,13,14,15,16,-2.0,inf,7.0,1.8e-06,6.1,nan,-2.0\n'
            '10,"he said ""x"", ok.png",12,13,14,15,16,17,18,19,20,21,22,23,inf,7.0,1.6999999999999998e-06,5.866666666666667,nan,-2.0,inf\n'
            '17,plain name.png,19,20,21,22,23,24,25,26,27,28,29,30,7.0,1.6e-06,5.633333333333333,nan,-2.0,inf,7.0\n'
        ),
        'summary.json': (
            '{\n'
            ' "mean_hcdr": 0.25,\n'
            ' "mean_vcdr": null,\n'
            ' "n": 3\n'
            '}\n'
        ),
    },
    'test_run': {
        'per_image.csv': (
            'index,name,disc_dice,cup_dice,disc_hd,disc_asd,cup_hd,cup_asd\n'
            '3,a.png,-2.0,inf,7.0,6e-07,2.1,nan\n'
            '10,"he said ""x"", ok.png",inf,7.0,5e-07,1.8666666666666667,nan,-2.0\n'
            '17,plain name.png,7.0,4e-07,1.6333333333333333,nan,-2.0,inf\n'
        ),
        'summary.json': (
            '{\n'
            ' "cup_dice": 0.5,\n'
            ' "disc_dice": NaN,\n'
            ' "n": 3\n'
            '}\n'
        ),
    },
    'uncertainty': {
        'uncertainty.csv': (
            'index,name,n_samples,n_defined,vcdr_mean,vcdr_std,vcdr_p05,vcdr_p95,hcdr_mean,hcdr_std,hcdr_p05,hcdr_p95,acdr_mean,acdr_std,acdr_p05,acdr_p95,disc_disagree_px,cup_disagree_px,disc_std_mean,cup_std_mean\n'
            '3,a.png,5,6,7.0,6e-07,2.1,nan,-2.0,inf,7.0,1.2e-06,4.1,nan,-2.0,inf,19,20,6.1,nan\n'
            '10,"he said ""x"", ok.png",12,13,5e-07,1.8666666666666667,nan,-2.0,inf,7.0,1.1e-06,3.8666666666666667,nan,-2.0,inf,7.0,26,27,nan,-2.0\n'
            '17,plain name.png,19,20,1.6333333333333333,nan,-2.0,inf,7.0,1e-06,3.6333333333333337,nan,-2.0,inf,7.0,1.6e-06,33,34,-2.0,inf\n'
        ),
    },
}


@pytest.mark.parametrize("program", sorted(WRITERS))
def test_writers_produce_the_recorded_bytes(program, tmp_path):
    got = _written(tmp_path, WRITERS[program])
    assert sorted(got) == sorted(EXPECTED[program])
    for f, text in EXPECTED[program].items():
        assert got[f] == text, (program, f)


def test_summaries_refuse_nan_except_the_test_runs(tmp_path):
    from wtpse_hip import calibration as C, segment as S, tables as T
    with pytest.raises(ValueError):
        S.write_measurements(str(tmp_path), [], {"mean_vcdr": NAN})
    with pytest.raises(ValueError):
        C.write_summary(str(tmp_path), {"n": NAN})
    T.write_json(str(tmp_path / "t.json"), {"b": NAN, "a": 1}, allow_nan=True)
    with open(tmp_path / "t.json") as f:
        text = f.read()
    assert text == '{\n "a": 1,\n "b": NaN\n}\n'
    with pytest.raises(ValueError):
        T.write_json(str(tmp_path / "t.json"), {"b": NAN}, allow_nan=False)


def test_shared_pair_round_trip(tmp_path):
    from wtpse_hip import tables as T
    columns, ints, texts = ("index", "name", "kind", "count", "value"), ("index", "count"), ("name", "kind")
    rows = rows_for(columns, ints, texts)
    path = str(tmp_path / "t.csv")
    T.write_csv(path, columns, rows, ints, texts)
    back = T.read_csv(path, ints, texts)
    assert [list(r) for r in back] == [list(columns)] * 3
    for a, b in zip(rows, back):
        assert b["name"] == a["name"] and b["kind"] == a["kind"] and type(b["index"]) is int and (b["index"], b["count"]) == (a["index"], a["count"])
        assert type(b["value"]) is float and (b["value"] == a["value"] or (math.isnan(b["value"]) and math.isnan(a["value"])))
    with open(path) as f:
        assert f.readline() == "index,name,kind,count,value\n" and f.readline().startswith("3,a.png,disc,6,")
    # only the column called "name" is quoted: another text column is written as it is
    T.write_csv(path, ("name", "kind"), [{"name": "a,b", "kind": "c,d"}], (), ("name", "kind"))
    with open(path) as f:
        assert f.read() == 'name,kind\n"a,b",c,d\n'
    T.write_csv(path, ("index",), [], ("index",))
    assert T.read_csv(path, ("index",)) == []

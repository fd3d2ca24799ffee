"""tools/timing.py without a GPU: the parent process of the learner-path timing tools (`run_children`: one child per index under a
time limit, nothing started after a child that fails or runs out of time) and the median (min-max) column (`fmt`)."""
from tools.timing import fmt, run_children

# a child: touches <dir>/<index>, then ends with the status the index picks from the list it is passed ("sleep": it outlives the limit)
CHILD = """import pathlib, sys, time
assert sys.argv[1] == "--child"
i, where, plan = int(sys.argv[2]), sys.argv[3], sys.argv[4].split(",")
pathlib.Path(where, str(i)).touch()
if plan[i] == "sleep":
    time.sleep(60)
sys.exit(int(plan[i]))
"""


def children(tmp_path, capsys, plan, limit=30):
    """(status, indices of the children that started, what was printed) of run_children over `plan`."""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    rc = run_children(str(script), len(plan), [str(tmp_path), ",".join(plan)], limit, lambda i: f"child {i}")
    return rc, sorted(int(p.name) for p in tmp_path.iterdir() if p.name.isdigit()), capsys.readouterr().out


def test_nothing_is_started_after_a_child_that_fails(tmp_path, capsys):
    assert children(tmp_path, capsys, ["0", "3", "0"]) == (3, [0, 1], "child 1 ended with status 3: nothing more is started\n")


def test_a_child_that_outlives_the_limit_counts_as_status_124(tmp_path, capsys):
    assert children(tmp_path, capsys, ["0", "sleep", "0"], limit=1) == (124, [0, 1], "child 1 ended with status 124: nothing more is started\n")


def test_all_children_run_when_none_fails(tmp_path, capsys):
    assert children(tmp_path, capsys, ["0", "0", "0"]) == (0, [0, 1, 2], "")


def test_a_single_child_is_named_without_a_sequel(tmp_path, capsys):
    assert children(tmp_path, capsys, ["1"]) == (1, [0], "child 0 ended with status 1\n")


def test_fmt_is_median_min_max():
    assert fmt([3.0, 1.25, 2.0, 10.0], 1) == "    2.5 (1.2-10.0)"
    assert fmt([0.5, 0.25, 4.0], 3) == "    0.500 (0.250-4.000)"

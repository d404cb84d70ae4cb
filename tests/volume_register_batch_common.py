"""The round scheduler of op_volume_register_batch_* restated (test infrastructure shared by tests/test_volume_register_batch_cpu.py and
tests/test_volume_register_batch_gpu.py).

Every cloud follows the single entries' loop on its own (tests/volume_register_common.py, loop): it is evaluated once per iteration and, when it
stopped after a step, once more at the pose that is returned.  In the restated loop that count is len(trace) + 1 whatever the status: the trace
receives one entry per solved iteration; a loop that ends on TOO_FEW_POINTS or SINGULAR ends on an evaluation without an entry and has no closing
one, every other loop has a closing one.  The library's result says the same number as iterations + 1.

The batch evaluates, in round r, exactly the clouds whose count exceeds r: all clouds start in round 0 and a cloud is evaluated in consecutive
rounds until it has had its last evaluation.  A round launches one registration kernel and one fold -- unless none of its clouds has a point."""


def rounds_of(evaluations):
    """evaluations[c]: how many evaluations cloud c's own loop makes -> the list of rounds, each the sorted list of the clouds evaluated in it"""
    return [[c for c, e in enumerate(evaluations) if e > r] for r in range(max(evaluations, default=0))]


def stats_of(evaluations, points):
    """-> the op_volume_register_batch_stats a batch of clouds with `points[c]` points and `evaluations[c]` evaluations must report"""
    rounds = rounds_of(evaluations)
    launched = [r for r in rounds if any(points[c] > 0 for c in r)]
    return dict(rounds=len(rounds), launches=2 * len(launched), evaluations=sum(evaluations), points=sum(points))


def workgroups(n):
    """the workgroups (and partial rows) a cloud of n points has, alone or in a batch: min(ceil(n / 256), 1024)"""
    return min((n + 255) // 256, 1024)

"""Rules over a call trace of tests/hostsan/hip_stub.cpp (HIP_STUB_TRACE): which stream a library call may queue on.

A trace is lines `launch <kernel> grid .. block .. s<k>`, `hipMemcpyAsync s<k>`, `hipMemsetAsync s<k>` (the WORK of the
rules below), `hipEventRecord s<k> e<j>`, `hipStreamWaitEvent s<k> e<j>`, `hipStreamSynchronize s<k>`,
`hipDeviceSynchronize`, and the harness's own `# ...` lines: `# step ...` (or any other mark) starts a step, one library
call; `# stream <label> s<k>` names a stream of the harness (`null` is the legacy default stream); `# caller <label>`
says which of them the context is on from there.  A trace without such lines (tests/golden/host_call_trace.txt) has its
contexts on `s0`.

R1  With the context on a stream U that is not the default stream, no call names the default stream.
R2  Within a step, for every stream L other than U that receives work:
    fork  before L's first work, L waits for an event recorded earlier IN THE SAME STEP on U or on a stream that was
          itself forked from U by this rule;
    join  after L's last work and before the step ends, U waits for an event recorded on L after that work -- directly,
          or through a stream that waited for it and is joined the same way --, or the step holds
          hipStreamSynchronize(L) or hipDeviceSynchronize after it.
    One path starts a stream without a fork by design: the upload stream of the drop-in Synthesis() carries host-to-
    device copies only, which depend on nothing queued before them; what they overwrite was read by the previous call
    of that stream's owner.  The rule it obeys, and which is checked instead of the fork: L carries nothing but
    hipMemcpyAsync in the step, and either L was never used before or, after the join of its previous use, the host
    synchronised the caller's stream (hipStreamSynchronize(U) or hipDeviceSynchronize).  The join rule applies to it
    as to any other stream.  How often the rule was applied is counted, and the tests pin the count: the number of
    drop-in Synthesis() steps in the recorded trace, none in a trace without that path.
After `# caller V` the same rules hold with V: every call is on V or on a stream forked from V.
"""
import re

WORK = ("launch ", "hipMemcpyAsync", "hipMemsetAsync")


def parse(line):
    """(kind, stream or None, event or None) of a call line."""
    m = re.search(r"(?: (s\d+))?(?: (e\d+))?$", line)
    stream, event = m.group(1), m.group(2)
    if line.startswith(WORK):
        return "work", stream, event
    return line.split(" ", 1)[0], stream, event


def check(lines, caller="s0"):
    """Every violation of R1 and R2 in `lines`, as (line number from 1, step, text); the counts of what was checked,
    `unforked` among them: how many times a stream started a step without a fork (the upload rule was applied)."""
    bad, names, null = [], {}, None
    step = "(before the first step)"
    stats = {"steps": 0, "side_streams": 0, "work": 0, "unforked": 0}
    # per step
    forked, unforked, recorded, last_work, waits, syncs = {caller}, set(), {}, {}, [], []
    # across steps, per stream: the line of the join of its last use, and the lines at which the host waited for the caller
    join_line, host_syncs = {}, []

    def joined(stream, after):
        """The first line at which work of `stream` queued up to line `after` is ordered into the caller's stream."""
        best = [i for i, s in syncs if i > after and s in (stream, None)]
        for i, s, rec in waits:
            if i > after and rec is not None and rec[0] == stream and rec[1] > after:
                at = i if s == caller else joined(s, i)
                if at is not None:
                    best.append(at)
        return min(best) if best else None

    def close(no):
        for L, at in last_work.items():
            if L == caller:
                continue
            stats["side_streams"] += 1
            j = joined(L, at)
            if j is None:
                bad.append((no, step, f"{L} is not joined into the caller's {caller} after its work at line {at}"))
            else:
                join_line[L] = j

    for no, line in enumerate(lines, 1):
        if line.startswith("#"):
            m = re.match(r"# stream (\S+) (s\d+)$", line)
            if m:
                names[m.group(1)] = m.group(2)
                null = names.get("null", null)
                continue
            close(no)
            forked, unforked, recorded, last_work, waits, syncs = {caller}, set(), {}, {}, [], []
            m = re.match(r"# caller (\S+)$", line)
            if m:
                caller = names[m.group(1)]
                forked = {caller}
                continue
            step = line[2:]
            stats["steps"] += 1
            continue
        kind, s, e = parse(line)
        if null is not None and caller != null and s == null:
            bad.append((no, step, f"R1: {line!r} names the default stream {null}"))
        if kind == "hipEventRecord":
            recorded[e] = (s, no)
        elif kind == "hipStreamWaitEvent":
            rec = recorded.get(e)
            waits.append((no, s, rec))
            if rec is not None and rec[0] in forked:
                forked.add(s)
        elif kind == "hipStreamSynchronize":
            syncs.append((no, s))
            if s == caller:
                host_syncs.append(no)
        elif kind == "hipDeviceSynchronize":
            syncs.append((no, None))
            host_syncs.append(no)
        elif kind == "work":
            stats["work"] += 1
            if s not in forked and s not in last_work:
                unforked.add(s)
                stats["unforked"] += 1
                if s in join_line and not any(i > join_line[s] for i in host_syncs):
                    bad.append((no, step, f"{s} starts without a fork from {caller} before its previous use is settled"))
            if s in unforked and not line.startswith("hipMemcpyAsync"):
                bad.append((no, step, f"{s} was not forked from {caller} and carries {line.split(' grid')[0]!r}"))
            last_work[s] = no
        else:
            bad.append((no, step, f"unknown trace line {line!r}"))
    close(len(lines) + 1)
    return bad, stats

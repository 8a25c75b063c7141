"""The GPU-free half of the engine's state file (host/state_file.hpp): header and
records written, parsed and laid out the same way for 1-, 2- and 3-D, one and
three bodies, both models; every mismatch and a truncated file refused with a
message that names the field; the temporary name and the rename."""
import os
import struct

import numpy as np
import pytest

HEADER, RECORD = 48, 32


@pytest.fixture(scope="module")
def H():
    from gcm_amd import _gcm_host
    return _gcm_host


def m_of(D, model):
    return D + D * (D + 1) // 2 if model == "elastic" else D + 1


def bodies_for(D, n, model):
    base = [[7], [5, 6], [3, 4, 5]][D - 1]
    return [(10 + 3 * k, model, m_of(D, model), [s + k for s in base]) for k in range(n)]


def data_for(body, seed):
    _, _, M, sizes = body
    bits = np.random.default_rng(seed).integers(0, 2 ** 64, size=tuple(sizes) + (M,), dtype=np.uint64)
    return bits.view(np.float64)


def write_file(H, path, D, bodies, steps=5, time=0.625, time_step=0.125, commit=True):
    w = H.StateFileWriter(str(path))
    w.write_header(D, steps, time, time_step, bodies)
    datas = []
    for k, b in enumerate(bodies):
        w.write_body_record(b)
        datas.append(data_for(b, k))
        w.write(datas[-1])
    if commit:
        w.commit()
    return w, datas


CASES = [(D, n, model) for D in (1, 2, 3) for n in (1, 3) for model in ("elastic", "acoustic")]


@pytest.mark.parametrize("D,n,model", CASES)
def test_round_trip_and_offsets(H, tmp_path, D, n, model):
    bodies = bodies_for(D, n, model)
    path = tmp_path / "state.gcmx"
    nan_time = float(np.array([0x7FF80000DEADBEEF], dtype=np.uint64).view(np.float64)[0])
    w, datas = write_file(H, path, D, bodies, steps=2 ** 40 + 3, time=nan_time, time_step=-0.0)
    # the layout, by hand
    want, at = [], HEADER
    for b, d in zip(bodies, datas):
        at += RECORD
        want.append(at)
        at += d.size * 8
    want.append(at)
    assert H.state_file_offsets(D, bodies) == want
    assert os.path.getsize(path) == want[-1] == w.written
    got = H.state_file_read(str(path))
    assert got["D"] == D and got["steps"] == 2 ** 40 + 3 and got["offsets"] == want
    assert [tuple(b) for b in got["bodies"]] == [tuple(b) for b in bodies]
    # the clock's doubles arrive as bits
    assert struct.pack("<d", got["time"]) == struct.pack("<d", nan_time)
    assert struct.pack("<d", got["time_step"]) == struct.pack("<d", -0.0)
    H.state_file_check(str(path), D, bodies)
    # little-endian, field by field
    raw = path.read_bytes()
    assert raw[:8] == b"GCMXSTAT"
    assert struct.unpack("<IIQqQQ", raw[8:HEADER]) == (1, D, n, 2 ** 40 + 3, 0x7FF80000DEADBEEF, 0x8000000000000000)
    for k, (b, d) in enumerate(zip(bodies, datas)):
        rec = struct.unpack("<QIIIIII", raw[want[k] - RECORD:want[k]])
        assert rec == (b[0], 0 if model == "elastic" else 1, b[2], *(b[3] + [1] * (3 - D)), 0)
        assert raw[want[k]:want[k] + d.size * 8] == d.tobytes()


def refused(H, path, D, bodies, field):
    with pytest.raises(H.GcmException) as err:
        H.state_file_check(str(path), D, bodies)
    assert field in str(err.value), (field, str(err.value))


@pytest.mark.parametrize("D,n,model", CASES)
def test_mismatches_name_the_field(H, tmp_path, D, n, model):
    bodies = bodies_for(D, n, model)
    path = tmp_path / "state.gcmx"
    write_file(H, path, D, bodies)
    last = n - 1
    change = lambda k, **kw: [tuple(kw.get(f, v) for f, v in zip(("id", "model", "M", "sizes"), b)) if i == k else b
                              for i, b in enumerate(bodies)]
    refused(H, path, D % 3 + 1, bodies, "D:")
    refused(H, path, D, bodies + [bodies[0]], "body count:")
    refused(H, path, D, bodies[:-1] if n > 1 else bodies * 2, "body count:")
    refused(H, path, D, change(last, id=99), f"body {last}: id:")
    other = "acoustic" if model == "elastic" else "elastic"
    refused(H, path, D, change(last, model=other), f"body {last}: model:")
    refused(H, path, D, change(0, M=bodies[0][2] + 1), "body 0: M:")
    for d in range(D):
        sizes = list(bodies[last][3])
        sizes[d] += 1
        refused(H, path, D, change(last, sizes=sizes), f"body {last}: sizes:")


def test_truncated_and_foreign_files_are_refused(H, tmp_path):
    D, bodies = 3, bodies_for(3, 3, "elastic")
    path = tmp_path / "state.gcmx"
    write_file(H, path, D, bodies)
    raw = path.read_bytes()
    offsets = H.state_file_offsets(D, bodies)
    cut = tmp_path / "cut.gcmx"

    def refused_file(data, field):
        cut.write_bytes(data)
        with pytest.raises(H.GcmException) as err:
            H.state_file_read(str(cut))
        assert field in str(err.value), (field, str(err.value))

    refused_file(raw[:-1], "truncated")                      # one byte short
    refused_file(raw[:offsets[1] + 8], "truncated")          # inside the second body's nodes
    refused_file(raw[:offsets[1] - 5], "truncated")          # inside the second body's record
    refused_file(raw[:HEADER - 1], "truncated")              # inside the header
    refused_file(raw[:HEADER], "body count")                 # no record at all
    refused_file(raw + b"\0", "size:")                       # one byte long
    refused_file(b"NOTASTAT" + raw[8:], "magic")
    refused_file(raw[:8] + struct.pack("<I", 2) + raw[12:], "version")
    refused_file(raw[:12] + struct.pack("<I", 4) + raw[16:], "D:")
    refused_file(raw[:24] + struct.pack("<q", -1) + raw[32:], "steps")
    bad_model = raw[:HEADER + 8] + struct.pack("<I", 7) + raw[HEADER + 12:]
    refused_file(bad_model, "body 0: model")
    bad_m = raw[:HEADER + 12] + struct.pack("<I", 0) + raw[HEADER + 16:]
    refused_file(bad_m, "body 0: M")
    with pytest.raises(H.GcmException, match="cannot open"):
        H.state_file_read(str(tmp_path / "absent.gcmx"))


def test_temporary_name_then_rename(H, tmp_path):
    D, bodies = 2, bodies_for(2, 1, "elastic")
    path = tmp_path / "deep" / "er" / "state.gcmx"
    # a first save
    w, _ = write_file(H, path, D, bodies, steps=1, commit=False)
    assert w.temporary_path == str(path) + ".tmp"
    assert os.path.exists(w.temporary_path) and not path.exists()
    w.commit()
    assert path.exists() and not os.path.exists(w.temporary_path)
    first = path.read_bytes()
    assert H.state_file_read(str(path))["steps"] == 1
    # a second save replaces it only at the rename
    w, _ = write_file(H, path, D, bodies, steps=2, commit=False)
    assert path.read_bytes() == first and os.path.exists(w.temporary_path)
    w.commit()
    assert H.state_file_read(str(path))["steps"] == 2 and not os.path.exists(w.temporary_path)
    second = path.read_bytes()
    # an interrupted save (no commit) leaves the final name as it was and no temporary file
    w, _ = write_file(H, path, D, bodies, steps=3, commit=False)
    del w
    import gc
    gc.collect()
    assert path.read_bytes() == second
    assert os.listdir(path.parent) == ["state.gcmx"]
    with pytest.raises(H.GcmException):
        w2, _ = write_file(H, path, D, bodies, steps=4)
        w2.commit()  # twice
    assert H.state_file_read(str(path))["steps"] == 4

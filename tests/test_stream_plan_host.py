"""The host side of an online-IK stream (csrc/stream_plan.h), compiled from the
header into a stand-alone program and run on the host (CPU only, plain C++17, no
HIP source): the stream's limits and their refusals, what the dataflow kernel
covers (a model outside it is a fallback, not an error), the dataflow step's plan
(frame counts, activation layout, phase table, counter words), the two weight
packers, and the check tik_stream_push makes of a frame before it takes it.

Everything is compared exactly: the plan only counts, and the packers only move
and split values. The rules are restated here in Python and numpy."""
import os
import subprocess

import numpy as np
import pytest

from test_fk_fold_host import CLANG, CSRC

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="the ROCm clang is not available")

TIK_E_INVALID = -1
V, HIDDEN, POSE = 17, 512, 66
G, T, H = 1, 2, 3                   # ONP_*
IDEN, CONV = 1, 2                   # ONR_*
MAXL, MAXC, MAXHC = 12, 256, 17     # ONL_*
IK_NET = [(64, 1), (64, 1), (128, 2), (128, 1), (128, 1), (128, 2), (256, 2), (256, 2)]
IK_WINS = (3, 9, 21, 22, 23, 64, 129)

# plan: argv = plan win_size V C0 feat hidden pose_dim, then cin cinp cout stride res per layer
#   refused  -> exit 3 and "<code> <message>"
#   else     -> "limits h W tout period ring_floats poses_floats", then "fallback <reason>" or
#               "plan act_floats act_bytes hpart pose ntasks trace_words cnt ncnt ticket done err words",
#               "L tin n_in n_out k32 gk32 x z out" per layer, "P kind layer nframes ngroups task0 cbase" per phase
# pack: argv = pack in out; in: int32 cin cinp cout stride res, float32 wt [cout][3 cout], wr [cout][cinp] (res conv),
#   wg [cout][cinp]; out: float32 K-concatenated rows, then for the temporal conv and for the gcn: int64 counts of
#   wf and wp, float32 wf, uint16 wp
# frame: argv = frame in; in: 51 float32 -> "<code of check_frame> <first_nonfinite> <message>"
SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "stream_plan.h"
using namespace tik_stream_plan;
static int plan(int argc, char** argv) {
    if (argc < 8 || (argc - 8) % 5) return 2;
    ModelShape m;
    const int win = atoi(argv[2]);
    m.V = atoi(argv[3]); m.C0 = atoi(argv[4]); m.feat = atoi(argv[5]); m.hidden = atoi(argv[6]); m.pose_dim = atoi(argv[7]);
    for (int a = 8; a < argc; a += 5)
        m.layers.push_back(LayerShape{atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]), atoi(argv[a + 4])});
    Limits lim;
    if (const int rc = stream_limits(m, win, lim)) {
        printf("%d %s\n", rc, tik_host::g_err.c_str());
        return 3;
    }
    printf("limits %d %d %d %lld %zu %zu\n", lim.h, lim.W, lim.tout, lim.period, lim.ring_floats, lim.poses_floats);
    const std::string why = coverage(m);
    Plan p;
    if (!why.empty() || !plan_dataflow(m, lim, p)) {
        printf("fallback %s\n", why.empty() ? "activation bytes" : why.c_str());
        return 0;
    }
    if (p.L.size() != m.layers.size() || p.ph.size() > (size_t)tik::ONL_MAXPH) return 4;
    printf("plan %lld %u %lld %lld %d %d %d %d %d %d %d %d\n", p.act_floats, p.act_bytes, p.hpart, p.pose, p.ntasks, p.trace_words,
           p.c.cnt, p.c.ncnt, p.c.ticket, p.c.done, p.c.err, p.c.words);
    for (const LayerPlan& l : p.L) printf("L %d %d %d %d %d %lld %lld %lld\n", l.tin, l.n_in, l.n_out, l.k32, l.gk32, l.x, l.z, l.out);
    for (const tik::OnlinePhase& q : p.ph) printf("P %d %d %d %d %d %d\n", q.kind, q.layer, q.nframes, q.ngroups, q.task0, q.cbase);
    return 0;
}
template <class T> static void put(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }
static int pack(int argc, char** argv) {
    FILE* fi = argc == 4 ? fopen(argv[2], "rb") : nullptr;
    if (!fi) return 2;
    LayerShape l;
    if (fread(&l, sizeof(int), 5, fi) != 5) return 2;
    std::vector<float> wt((size_t)l.cout * 3 * l.cout), wr(l.res == tik::ONR_CONV ? (size_t)l.cout * l.cinp : 0), wg((size_t)l.cout * l.cinp);
    for (std::vector<float>* v : {&wt, &wr, &wg})
        if (fread(v->data(), sizeof(float), v->size(), fi) != v->size()) return 2;
    fclose(fi);
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) return 2;
    const std::vector<float> w = concat_k(l, wt, wr);
    put(fo, w);
    std::vector<float> wf;
    std::vector<unsigned short> wp;
    for (int gcn = 0; gcn < 2; ++gcn) {
        pack_rows(gcn ? wg : w, l.cout, gcn ? l.cinp : tconv_k(l), wf, wp);
        const long long n[2] = {(long long)wf.size(), (long long)wp.size()};
        fwrite(n, 8, 2, fo);
        put(fo, wf);
        put(fo, wp);
    }
    fclose(fo);
    return 0;
}
static int frame(int argc, char** argv) {
    FILE* fi = argc == 3 ? fopen(argv[2], "rb") : nullptr;
    if (!fi) return 2;
    float f[FRAME + 1];
    const size_t n = fread(f, sizeof(float), FRAME + 1, fi);
    fclose(fi);
    if (n != FRAME) return 2;
    f[FRAME] = 0.f;
    const int rc = check_frame(f);
    printf("%d %d %s\n", rc, first_nonfinite(f, FRAME), rc ? tik_host::g_err.c_str() : "");
    return 0;
}
int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) return plan(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "frame")) return frame(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "pack")) return pack(argc, argv);
    return 2;
}
'''


def build_program(out_dir, extra_flags=()):
    src = os.path.join(out_dir, "stream_plan_main.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    exe = os.path.join(out_dir, "stream_plan_main")
    r = subprocess.run([CLANG, "-O1", "-std=c++17", "-Wall", "-Werror", *extra_flags, f"-I{CSRC}", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(str(tmp_path_factory.mktemp("stream_plan")))


def net(couts_strides, c0=3):
    """(cout, stride) blocks -> (cin, cinp, cout, stride, res) as the fold gives them."""
    out, c = [], c0
    for co, s in couts_strides:
        out.append((c, (c + 3) // 4 * 4, co, s, CONV if c != co or s != 1 else IDEN))
        c = co
    return out


def model(layers, hidden=HIDDEN, pose_dim=POSE, feat=None, v=V, c0=3):
    return dict(layers=layers, V=v, C0=c0, feat=V * layers[-1][2] if feat is None else feat, hidden=hidden, pose_dim=pose_dim)


def run_plan(exe, m, win):
    """-> ("refused", code, message) | ("fallback", limits, reason) | ("plan", limits, plan)"""
    args = [win, m["V"], m["C0"], m["feat"], m["hidden"], m["pose_dim"]] + [x for l in m["layers"] for x in l]
    r = subprocess.run([exe, "plan"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    if r.returncode == 3:
        code, _, msg = r.stdout.strip().partition(" ")
        return "refused", int(code), msg
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0].startswith("limits ")
    lim = dict(zip(("h", "W", "tout", "period", "ring_floats", "poses_floats"), map(int, lines[0].split()[1:])))
    if lines[1].startswith("fallback "):
        return "fallback", lim, lines[1][len("fallback "):]
    p = dict(zip(("act_floats", "act_bytes", "hpart", "pose", "ntasks", "trace_words", "cnt", "ncnt", "ticket", "done", "err", "words"),
                 map(int, lines[1].split()[1:])))
    p["L"] = [tuple(map(int, ln.split()[1:])) for ln in lines[2:] if ln.startswith("L ")]
    p["P"] = [tuple(map(int, ln.split()[1:])) for ln in lines[2:] if ln.startswith("P ")]
    assert 2 + len(p["L"]) + len(p["P"]) == len(lines)
    return "plan", lim, p


def expected_limits(m, win):
    h = win // 2
    W = t = 2 * h + 1
    for *_, s, _ in m["layers"]:
        t = (t - 1) // s + 1
    return dict(h=h, W=W, tout=t, period=2 * W, ring_floats=W * V * 3, poses_floats=t * POSE)


def expected_plan(m, win):
    """The dataflow step as online.h describes it: output frame t of a stride-s layer reads input
    frames s t - 1 .. s t + 1; walk back from the one frame the head reads."""
    layers, W = m["layers"], 2 * (win // 2) + 1
    tin, t = [], W
    for *_, s, _ in layers:
        tin.append(t)
        t = (t - 1) // s + 1
    n_in, n_out, need = [0] * len(layers), [0] * len(layers), 1
    for l in reversed(range(len(layers))):
        n_out[l] = need
        need = n_in[l] = min(tin[l], layers[l][3] * (need - 1) + 2)
    L, P, q, task = [], [], 0, 0
    for l, (ci, cip, co, s, res) in enumerate(layers):
        z, out = q, q + n_in[l] * V * co
        q = out + n_out[l] * V * co
        kt = 3 * co + (cip if res == CONV else 0)
        L.append((tin[l], n_in[l], n_out[l], -(-kt // 32), -(-cip // 32), L[-1][7] if l else -1, z, out))
        for kind, nf in ((G, n_in[l]), (T, n_out[l])):
            P.append((kind, l, nf, co // 16, task, 0))
            task += nf * (co // 16)
    P.append((H, len(layers) - 1, 1, m["hidden"] // 16, task, 0))
    task += m["hidden"] // 16
    hpart = q
    pose = hpart + m["hidden"] // 16 * m["pose_dim"]
    tot = pose + (m["pose_dim"] + 3) // 4 * 4
    return dict(act_floats=tot, act_bytes=4 * tot, hpart=hpart, pose=pose, ntasks=task, trace_words=8 * task, cnt=0, ncnt=1, ticket=1,
                done=2, err=3, words=4, L=L, P=P)


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("win", IK_WINS)
def test_ik_net_plan(program, win):
    m = model(net(IK_NET))
    kind, lim, p = run_plan(program, m, win)
    assert kind == "plan"
    assert lim == expected_limits(m, win)
    assert p == expected_plan(m, win)
    # the values of the current rules, pinned
    W = lim["W"]
    if W >= 23:
        assert [l[1] for l in p["L"]] == [22, 21, 20, 10, 9, 8, 4, 2]
    assert p["ntasks"] == {3: 272, 9: 640, 21: 1132}.get(W, 1136)
    assert p["act_floats"] == {3: 67460, 9: 167556, 21: 301380}.get(W, 302468)
    # the buffers do not overlap and fill the total; tasks are numbered without gaps
    spans = sorted([(l[6], l[1] * V * c[2]) for l, c in zip(p["L"], m["layers"])] + [(l[7], l[2] * V * c[2]) for l, c in zip(p["L"], m["layers"])] +
                   [(p["hpart"], HIDDEN // 16 * POSE), (p["pose"], 68)])
    assert spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:])) and sum(spans[-1]) == p["act_floats"]
    assert all(a[4] + a[2] * a[3] == b[4] for a, b in zip(p["P"], p["P"][1:])) and p["P"][-1][4] + p["P"][-1][3] == p["ntasks"]
    assert sorted({p["cnt"], p["ticket"], p["done"], p["err"]}) == list(range(p["words"]))


@pytest.mark.parametrize("c1", [48, 80])
def test_k_steps_where_k_is_no_multiple_of_32(program, c1):
    """The nets of test_online_identity_block_c_mod_32_eq_16: 3 C = 144 / 240 (+ 4 with layer 0's residual conv)."""
    m = model(net([(c1, 1), (c1, 1), (c1, 1), (128, 2), (128, 1), (128, 2), (256, 2), (256, 2)]))
    kind, lim, p = run_plan(program, m, 64)
    assert kind == "plan" and lim == expected_limits(m, 64) and p == expected_plan(m, 64)
    k32, gk32 = {48: (5, 2), 80: (8, 3)}[c1]
    assert [(l[3], l[4]) for l in p["L"][:4]] == [(k32, 1), (k32, gk32), (k32, gk32), (12 + gk32, gk32)]


# ---------------------------------------------------------------- refusals and fallbacks
REFUSED = {
    "win_size 0": (0, POSE, "win_size 0 is not positive"),
    "win_size negative": (-3, POSE, "win_size -3 is not positive"),
    "2W past 2^29": (1 << 28, POSE, f"win_size {1 << 28} gives a ring of {(1 << 28) + 1} frames, and twice that exceeds 2^29"),
    "pose_dim 60": (9, 60, "the model's pose width is 60 (rows of pose_regressor.3); a stream returns 66 floats per pose"),
    "pose_dim 72": (9, 72, "the model's pose width is 72 (rows of pose_regressor.3); a stream returns 66 floats per pose"),
    "backbone only": (9, 0, "backbone-only model handle"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals(program, case):
    win, pose_dim, want = REFUSED[case]
    kind, code, msg = run_plan(program, model(net(IK_NET), pose_dim=pose_dim), win)
    print(f"{case}: {code} {msg}")
    assert kind == "refused" and code == TIK_E_INVALID
    assert msg == "tik_stream_create: " + want


def test_largest_window(program):
    """2 W = 2^29 - 2: the last window stream_next_count's divisor allows; the IK net's plan does not grow with it."""
    m, win = model(net(IK_NET)), (1 << 28) - 1
    kind, lim, p = run_plan(program, m, win)
    assert kind == "plan" and lim == expected_limits(m, win) and lim["period"] == (1 << 29) - 2
    assert p == expected_plan(m, win) and p["ntasks"] == 1136


DEEP = [(256, 4)] * 10   # 10 stride-4 layers: the walk back grows 4x per layer while the window allows it
FALLBACK = {
    "13 layers": (model(net([(64, 1)] * 12 + [(256, 1)])), 9),
    "cout 272": (model(net(IK_NET[:-1] + [(272, 2)])), 9),
    "cout 24": (model(net([(24, 1)] + IK_NET[1:])), 9),
    "hidden 520": (model(net(IK_NET), hidden=520), 9),
    "feat % 4": (model(net(IK_NET), feat=V * 256 + 2), 9),
    "activation bytes": (model(net(DEEP)), 1 << 21),
}


@pytest.mark.parametrize("case", list(FALLBACK))
def test_fallbacks_are_not_errors(program, case):
    m, win = FALLBACK[case]
    kind, lim, why = run_plan(program, m, win)
    print(f"{case}: {why}")
    assert kind == "fallback" and lim == expected_limits(m, win)
    if case == "activation bytes":
        assert why == "activation bytes" and expected_plan(m, win)["act_bytes"] >= 2 ** 31
        # the same chain at a window where the buffer fits is planned
        kind, lim, p = run_plan(program, m, 1 << 16)
        assert kind == "plan" and p == expected_plan(m, 1 << 16) and p["act_bytes"] < 2 ** 31


def test_limits_of_coverage(program):
    """The last shapes inside: 12 layers, 256 channels, the widest head."""
    m = model(net([(64, 1)] * 11 + [(256, 1)]), hidden=MAXHC * 256)
    kind, lim, p = run_plan(program, m, 64)
    assert kind == "plan" and p == expected_plan(m, 64) and len(p["P"]) == 2 * MAXL + 1


# ---------------------------------------------------------------- the packers
def bf16_rne(x):
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def expected_pack(w, cout, kt):
    """fp32 rows zero-padded to 32-steps, and their bf16x3 planes [cout/16][K32][3][64][8]: lane ln of a
    (16 rows x 32 K) step holds row ln % 16, K 8 (ln / 16) .. + 7."""
    k32 = -(-kt // 32)
    wf = np.zeros((cout, 32 * k32), np.float32)
    wf[:, :kt] = w.reshape(cout, kt)
    p0 = bf16_rne(wf)
    r1 = wf - bf16_to_f32(p0)
    p1 = bf16_rne(r1)
    p2 = bf16_rne(r1 - bf16_to_f32(p1))
    wp = np.zeros((cout // 16, k32, 3, 64, 8), np.uint16)
    for pl, plane in enumerate((p0, p1, p2)):
        for ln in range(64):
            for cg in range(cout // 16):
                for sk in range(k32):
                    wp[cg, sk, pl, ln] = plane[16 * cg + ln % 16, 32 * sk + 8 * (ln // 16):32 * sk + 8 * (ln // 16) + 8]
    return wf.ravel(), wp.ravel()


@pytest.mark.parametrize("cin,cout,stride", [(3, 16, 1), (48, 48, 1), (16, 32, 2), (32, 32, 1)])
def test_packers(program, tmp_path, cin, cout, stride):
    """K = 52 and 112 with a residual conv, 144 and 96 without; gcn K = 4, 48, 16, 32."""
    (ci, cip, co, s, res), = net([(cout, stride)], c0=cin)
    rng = np.random.default_rng(cin * 1000 + cout)
    scale = lambda n: (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
    wt, wr, wg = scale(co * 3 * co), scale(co * cip if res == CONV else 0), scale(co * cip)
    wg[::7] = 0.0
    fin, fout = str(tmp_path / "pack.in"), str(tmp_path / "pack.out")
    with open(fin, "wb") as f:
        f.write(np.array([ci, cip, co, s, res], np.int32).tobytes() + wt.tobytes() + wr.tobytes() + wg.tobytes())
    r = subprocess.run([program, "pack", fin, fout], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = open(fout, "rb").read()
    kt = 3 * co + (cip if res == CONV else 0)
    w = np.concatenate([wt.reshape(co, 3 * co)] + ([wr.reshape(co, cip)] if res == CONV else []), axis=1)
    got_w = np.frombuffer(raw, np.float32, co * kt)
    assert np.array_equal(got_w.view(np.uint32), w.ravel().view(np.uint32))
    pos = 4 * co * kt
    for rows, k in ((w, kt), (wg, cip)):
        nf, npl = np.frombuffer(raw, np.int64, 2, pos)
        wf = np.frombuffer(raw, np.float32, nf, pos + 16)
        wp = np.frombuffer(raw, np.uint16, npl, pos + 16 + 4 * nf)
        pos += 16 + 4 * nf + 2 * npl
        want_f, want_p = expected_pack(rows, co, k)
        assert nf == want_f.size and npl == want_p.size
        assert np.array_equal(wf.view(np.uint32), want_f.view(np.uint32))
        assert np.array_equal(wp, want_p)
        # the three planes add up to the value (normal fp32 values, and 0)
        pl = bf16_to_f32(wp.reshape(co // 16, -1, 3, 64, 8)).astype(np.float64).sum(axis=2)
        back = np.zeros_like(want_f.reshape(co, -1))
        for ln in range(64):
            for cg in range(co // 16):
                for sk in range(pl.shape[1]):
                    back[16 * cg + ln % 16, 32 * sk + 8 * (ln // 16):32 * sk + 8 * (ln // 16) + 8] = pl[cg, sk, ln]
        assert np.array_equal(back, want_f.reshape(co, -1))
    assert pos == len(raw)


# ---------------------------------------------------------------- the pushed frame
def run_frame(exe, tmp_path, f):
    """-> (code, index of the first non-finite value or -1, message)"""
    fin = str(tmp_path / "frame.in")
    np.asarray(f, np.float32).tofile(fin)
    r = subprocess.run([exe, "frame", fin], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    code, idx, msg = r.stdout.rstrip("\n").split(" ", 2)
    return int(code), int(idx), msg


def test_finite_frames_pass(program, tmp_path):
    """Every finite float32 passes: zeros of both signs, subnormals, the largest values."""
    tiny, big = np.finfo(np.float32).tiny, np.finfo(np.float32).max
    f = np.random.default_rng(1).normal(0, 0.3, 51).astype(np.float32)
    f[:8] = [0.0, -0.0, tiny, -tiny, tiny / 4, np.float32(1e-45), big, -big]
    assert run_frame(program, tmp_path, f) == (0, -1, "")
    assert run_frame(program, tmp_path, np.zeros(51)) == (0, -1, "")


@pytest.mark.parametrize("where", [0, 1, 32, 50])
@pytest.mark.parametrize("name,bits", [("NaN", 0x7fc00000), ("NaN", 0xffc00001), ("NaN", 0x7f800001), ("infinite", 0x7f800000),
                                       ("infinite", 0xff800000)])
def test_non_finite_frames_are_refused(program, tmp_path, where, name, bits):
    """Quiet, negative and signalling NaNs and both infinities, at the first, an inner
    and the last of the 51 values: TIK_E_INVALID, naming the first of them."""
    f = np.random.default_rng(2).normal(0, 0.3, 51).astype(np.float32)
    f.view(np.uint32)[where] = bits
    f.view(np.uint32)[50] = bits if where == 50 else 0x7fc00000     # a later one does not change the answer
    code, idx, msg = run_frame(program, tmp_path, f)
    assert (code, idx) == (TIK_E_INVALID, where)
    assert msg == f"tik_stream_push: frame value {where} (joint {where // 3}, coordinate {where % 3}) is {name}; the frame was not appended"

"""The slab reducer (csrc/elementwise_bwd.hip: k_slab_reduce / k_slab_reduce_link) alone, against float64 sums on the host.

dst[i] += sum_{s < nslab} slab[s * stride + i], i < count.  The kernels are driven through `tcvn_debug_slab_reduce`, an entry of the
validation build only, in ONE child process for all cases (tests/variant_utils.run_on_debug_build); the tests below assert on what it
returns.

Cases: every (count, nslab, stride, dst alignment) of
    count   1, 27, 33, 128, 1027, 16 384, 36 864
    nslab   1, 7, 8, 9, 64, 255, 512, 513, 1024
    stride  = count, and one larger stride per count (27 -> 32: the 3x3 bias rows; some keep the rows 16-B aligned, some do not)
    dst     16-B aligned, and 4 B behind that
    slab    16-B aligned; and, for nslab 9 and 513 of every count, 4 B behind that (rows that take scalar loads whatever the stride)
and two launches of several jobs: four jobs of unlike sizes with a BatchNorm link in the same launch, and three jobs whose middle
one is empty.

Every float of the slab buffer outside [0, nslab) x [0, count) -- the columns between count and stride, two rows behind the last
slab -- is NaN, and dst sits between NaN guard elements that must come back untouched: a read or a write outside the job shows.

Tolerance, derived (not tuned): |got - ref| <= nslab * 2^-23 * sum_s |x_s| per element.  The bound has no term for what dst held, so
dst is pre-filled with HALF the first slab (the kernel accumulates: an exact, nonzero start value that the bound covers): every
floating-point addition on an element's path rounds by at most 2^-24 of a partial sum that is at most 1.5 * sum_s |x_s|, and at most
nslab of the additions on a path have two nonzero operands, so the error is below 1.5 * nslab * 2^-24 * sum|x| < the bound.

Every case runs twice from the same start; the two results must be bit-identical (fixed summation order, no atomics)."""
import pytest

pytestmark = pytest.mark.gpu

COUNTS = [1, 27, 33, 128, 1027, 16384, 36864]
NSLABS = [1, 7, 8, 9, 64, 255, 512, 513, 1024]
WIDE = {1: 4, 27: 32, 33: 40, 128: 131, 1027: 1032, 16384: 16388, 36864: 36867}      # the larger stride of each count

BODY = r"""
import ctypes as C
import numpy as np
from transformercvn.hip import _lib
fn = _lib.lib.tcvn_debug_slab_reduce
fn.restype = C.c_int
P = C.c_void_p
fn.argtypes = [C.c_int, C.POINTER(P), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(P),
               C.c_int, C.c_int, P, P, C.c_longlong, C.c_float, P, P, P, P, P, P, C.c_int, P]
COUNTS, NSLABS, WIDE = %(counts)r, %(nslabs)r, %(wide)r
NAN = float("nan")
rng = np.random.default_rng(5)
base = rng.standard_normal(1026 * 36868 + 64, dtype=np.float32)      # one pool of values; every case reads a prefix of it
base_gpu = torch.from_numpy(base).cuda()
GUARD = 8


def make_job(count, nslab, stride, misalign, slab_off=0):
    # slab rows [nslab + 2][stride] from the pool, NaN outside the job; dst between NaN guards, pre-filled with half of slab 0
    # (slab_off = 1: the rows start one float behind a 16-B aligned, NaN-filled element)
    raw = torch.full(((nslab + 2) * stride + 4,), NAN, device="cuda")
    assert raw.data_ptr() %% 16 == 0
    buf = raw[slab_off:slab_off + (nslab + 2) * stride]
    buf.copy_(base_gpu[:(nslab + 2) * stride])
    buf = buf.view(nslab + 2, stride)
    buf[:, count:] = NAN
    buf[nslab:, :] = NAN
    dst = torch.full((GUARD + 1 + count + GUARD,), NAN, device="cuda")
    lo = GUARD + misalign
    dst[lo:lo + count] = 0.5 * buf[0, :count]
    assert buf.data_ptr() %% 16 == 4 * slab_off and dst.data_ptr() %% 16 == 0
    return buf, dst, lo


def host_ref(count, nslab, stride):
    x = base[:nslab * stride].reshape(nslab, stride)[:, :count].astype(np.float64)
    return 0.5 * x[0] + x.sum(0), np.abs(x).sum(0)


def launch(jobs, link=None):
    n = len(jobs)
    slab = (P * 4)(*[j["buf"].data_ptr() for j in jobs])
    dst = (P * 4)(*[j["dst"].data_ptr() + 4 * j["lo"] for j in jobs])
    ns = (C.c_int * 4)(*[j["nslab"] for j in jobs])
    cnt = (C.c_longlong * 4)(*[j["count"] for j in jobs])
    strd = (C.c_longlong * 4)(*[j["stride"] for j in jobs])
    if link is None:
        rc = fn(n, slab, ns, cnt, strd, dst, 0, 0, None, None, 0, 0.0, None, None, None, None, None, None, 0, None)
    else:
        t = link
        rc = fn(n, slab, ns, cnt, strd, dst, t["C"], t["nblk"], t["part"].data_ptr(), t["bstat"].data_ptr(), t["count"], t["eps"],
                t["gamma"].data_ptr(), t["dgamma"].data_ptr(), t["dbeta"].data_ptr(), t["dslope"].data_ptr(), t["P"].data_ptr(),
                t["Q"].data_ptr(), 0, None)
    assert rc == 0, rc


def job(count, nslab, stride, misalign, slab_off=0):
    buf, dst, lo = make_job(count, nslab, stride, misalign, slab_off)
    return dict(buf=buf, dst=dst, lo=lo, count=count, nslab=nslab, stride=stride)


def judge(j, got, ref, sabs):
    # -> (worst error / bound, guards untouched, slab buffer untouched is implied: the kernel has no store to it)
    lo, count = j["lo"], j["count"]
    g = got.cpu().numpy()
    body = g[lo:lo + count].astype(np.float64)
    bound = j["nslab"] * 2.0 ** -23 * sabs
    ok = np.abs(body - ref) <= bound
    ratio = float(np.max(np.abs(body - ref) / np.maximum(bound, 1e-300)))
    guards = bool(np.isnan(g[:lo]).all() and np.isnan(g[lo + count:]).all())
    return dict(all_within=bool(ok.all()), finite=bool(np.isfinite(body).all()), worst=ratio, guards=guards)


single = {}
for count in COUNTS:
    for nslab in NSLABS:
        for stride in (count, WIDE[count]):
            ref, sabs = host_ref(count, nslab, stride)
            for mis, slab_off in ((0, 0), (1, 0)) + (((0, 1), (1, 1)) if nslab in (9, 513) else ()):
                runs = []
                for rep in range(2):
                    j = job(count, nslab, stride, mis, slab_off)
                    launch([j])
                    runs.append(j["dst"].clone())
                torch.cuda.synchronize()
                r = judge(j, runs[0], ref, sabs)
                r["repeat_identical"] = bool(torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)))
                single[(count, nslab, stride, mis, slab_off)] = r


def multi(specs, link_C):
    out = []
    for rep in range(2):
        jobs = [job(*s) for s in specs]
        link = None
        if link_C:
            g = torch.Generator().manual_seed(9)
            nblk = 40
            link = dict(C=link_C, nblk=nblk, count=5000, eps=1e-5,
                        part=torch.randn(nblk, link_C, 3, generator=g, dtype=torch.float64).cuda(),
                        bstat=torch.stack([torch.randn(link_C, generator=g, dtype=torch.float64),
                                           torch.rand(link_C, generator=g, dtype=torch.float64) + 0.5], 1).contiguous().cuda(),
                        gamma=(torch.rand(link_C, generator=g) + 0.5).cuda())
            for k in ("dgamma", "dbeta", "dslope"):
                link[k] = torch.randn(link_C, generator=g).cuda()
            link["P"] = torch.full((link_C,), NAN, device="cuda")
            link["Q"] = torch.full((link_C,), NAN, device="cuda")
            start = {k: link[k].clone() for k in ("dgamma", "dbeta", "dslope")}
        launch(jobs, link)
        torch.cuda.synchronize()
        res = []
        for j in jobs:
            if j["count"] == 0:
                res.append(None)
                continue
            ref, sabs = host_ref(j["count"], j["nslab"], j["stride"])
            res.append((judge(j, j["dst"], ref, sabs), j["dst"].clone().view(torch.int32).cpu()))
        lk = None
        if link_C:
            # float64 on the host: the formulas in csrc/bn_link.h
            part, bstat = link["part"].cpu(), link["bstat"].cpu()
            s1, t2, s3 = part[:, :, 0].sum(0), part[:, :, 1].sum(0), part[:, :, 2].sum(0)
            mu, var = bstat[:, 0], bstat[:, 1]
            r = 1.0 / torch.sqrt(var + float(np.float32(1e-5)))
            dgamma = r * (t2 - mu * s1)
            sc = link["gamma"].cpu().double() * r
            M = 5000.0
            want = dict(dgamma=start["dgamma"].cpu().double() + dgamma.float().double(),
                        dbeta=start["dbeta"].cpu().double() + s1.float().double(),
                        dslope=start["dslope"].cpu().double() + s3.float().double(),
                        P=-sc * dgamma * r / M, Q=-sc * s1 / M + sc * dgamma * r * mu / M)
            lk = {k: (link[k].cpu().double(), want[k]) for k in want}
            lk["bits"] = {k: link[k].clone().view(torch.int32).cpu() for k in want}
        out.append((res, lk))
    return out


# four jobs of unlike sizes (3x3 weights, 1x1 bias, 3x3 bias rows of stride 32, an odd unaligned job) and a link in one launch
result = dict(single=single,
              four_link=multi([(36864, 40, 36864, 0), (128, 40, 128, 0), (27, 40, 32, 0), (1027, 513, 1027, 1)], 128),
              empty_middle=multi([(16384, 9, 16384, 0), (0, 0, 0, 0), (33, 255, 40, 1)], 0))
""" % dict(counts=COUNTS, nslabs=NSLABS, wide=WIDE)


@pytest.fixture(scope="module")
def reduced():
    from variant_utils import run_on_debug_build
    return run_on_debug_build(BODY, {})


@pytest.mark.parametrize("count", COUNTS)
def test_single_jobs_match_float64_sums(reduced, count):
    worst, n_cases = 0.0, 0
    for nslab in NSLABS:
        for stride in (count, WIDE[count]):
            for mis, slab_off in ((0, 0), (1, 0)) + (((0, 1), (1, 1)) if nslab in (9, 513) else ()):
                case = (count, nslab, stride, mis, slab_off)
                r = reduced["single"][case]
                worst, n_cases = max(worst, r["worst"]), n_cases + 1
                assert r["finite"], (case, "a NaN from outside the job reached the sum")
                assert r["all_within"], (case, r["worst"])
                assert r["guards"], (case, "dst written outside [0, count)")
                assert r["repeat_identical"], (case, "two runs differ")
    print(f"count {count}: worst error / bound over {n_cases} cases = {worst:.3f}")


def _check_multi(runs, live):
    (res0, lk0), (res1, lk1) = runs
    assert [r is not None for r in res0] == live
    for (a, b) in zip(res0, res1):
        if a is None:
            continue
        (ja, bits_a), (jb, bits_b) = a, b
        assert ja["finite"] and ja["all_within"] and ja["guards"], ja
        assert (bits_a == bits_b).all(), "two runs differ"
    return lk0, lk1


def test_four_unlike_jobs_and_a_link_in_one_launch(reduced):
    lk0, lk1 = _check_multi(reduced["four_link"], [True, True, True, True])
    for k in ("dgamma", "dbeta", "dslope", "P", "Q"):
        got, want = lk0[k]
        # fp32 results of float64 arithmetic: one rounding of the increment, one of the accumulating add
        err = (got - want).abs().max().item()
        scale = want.abs().max().item()
        print(f"link {k}: max abs error {err:.3e} (scale {scale:.3e})")
        assert err <= 4 * 2.0 ** -24 * scale, (k, err, scale)
    for k in lk0["bits"]:
        assert (lk0["bits"][k] == lk1["bits"][k]).all(), k


def test_an_empty_job_in_the_middle_is_skipped(reduced):
    _check_multi(reduced["empty_middle"], [True, False, True])

"""The forwarding step on the device (cgpu_forward_v4 / _v6, Engine.forward_v4 /
_v6, forward= on the classify calls).

The compiled-reference harnesses keep cilium_lxc and the tunnel map empty, so
the reference is the restatement in tests/forward_cases.py, which the literal
table there pins (tests/test_forward_cpu.py).  Outputs are compared column by
column, bit for bit: the step is integer-only."""
import numpy as np
import pytest

from cilium_amd import build, layouts as L, synth
from forward_cases import (CASES, ENDPOINT_F_HOST, LXC, NETDEV, World, batch_world, build_batch, case_columns,
                           categories, engine_cfg, fwd_kwargs, ip4, ip6, key4, key6, literal_world, load_world,
                           restate)

pytestmark = pytest.mark.gpu
COLS = ("action", "ret", "ifindex", "arg")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a device"
    build.build()
    return torch


def _engine(**kw):
    from cilium_amd.engine import Engine
    return Engine(device=0, **kw)


def _dev(torch, b, v6, offset=0):
    """the batch's columns as device tensors (None stays None); offset: the
    IPv6 address column starts that many bytes into its allocation"""
    d = {}
    for k, x in b.items():
        if x is None:
            d[k] = None
        elif k == "daddr" and v6:
            n = len(x)
            raw = torch.zeros(16 * n + 16, dtype=torch.uint8, device="cuda")
            raw[offset:offset + 16 * n] = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()
            d[k] = raw[offset:offset + 16 * n].view(n, 16)
        elif k in ("daddr", "tunnel"):
            d[k] = torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).cuda()
        else:
            d[k] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return d


def _np(out):
    r = {"action": out["action"].cpu().numpy(), "ret": out["ret"].cpu().numpy() if out.get("ret") is not None else None}
    for k in ("ifindex", "arg"):
        r[k] = out[k].cpu().numpy().view(np.uint32) if out.get(k) is not None else None
    return r


def _run(torch, e, w, mode, v6, b, offset=0, out=None):
    d = _dev(torch, b, v6, offset)
    fn = e.forward_v6 if v6 else e.forward_v4
    o = fn(d["daddr"], verdict=d.get("verdict"), tunnel=d.get("tunnel"), flags=d.get("flags"), ttl=d.get("ttl"),
           out=out, **fwd_kwargs(w, mode))
    torch.cuda.synchronize()
    return _np(o)


def _same(got, exp, msg):
    for k in COLS:
        if got[k] is not None:
            np.testing.assert_array_equal(got[k], exp[k], err_msg=f"{msg}: {k}")


@pytest.fixture(scope="module")
def batch_engine(torch_cuda):
    w = batch_world()
    e = _engine(**engine_cfg(w))
    load_world(e, w)
    e.commit()
    yield e
    e.close()


# --------------------------------------------------------------------------
# 1. both programs, both families, with and without ENCAP, every row
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("encap", [True, False], ids=["encap", "noencap"])
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("mode", [LXC, NETDEV], ids=["lxc", "netdev"])
def test_batches_match_the_restatement(torch_cuda, batch_engine, mode, v6, encap, n):
    w = batch_world(encap)
    b = build_batch(w, v6, n)
    if n >= 257:  # every row of the decision lists is in the batch
        for name, m in categories(w, mode, v6, b).items():
            assert m.any(), name
    _same(_run(torch_cuda, batch_engine, w, mode, v6, b), restate(w, mode, v6, **b), f"mode {mode} v6 {v6} n {n}")


def test_netdev_v6_gate_value_zero(torch_cuda):
    """inside the IPv6 netdev gate there is one tunnel key, ROUTER_IP's /96: its
    value with ip4 == 0 is still an OVERLAY, arg 0"""
    w = literal_world()
    w.tun[key6(ip6("fd00::"))] = key4(0)
    e = _engine(**engine_cfg(w))
    load_world(e, w)
    e.commit()
    b = dict(daddr=np.frombuffer(ip6("fd00::77") + ip6("fd01::77"), np.uint8).reshape(2, 16).copy(),
             tunnel=np.zeros(2, np.uint32), ttl=np.array([1, 64], np.uint8))
    got = _run(torch_cuda, e, w, NETDEV, True, b)
    assert got["action"].tolist() == [5, 6] and got["arg"].tolist() == [0, 0]
    assert got["ifindex"].tolist() == [22, 0]
    _same(got, restate(w, NETDEV, True, **b), "router /96 -> 0")
    e.close()


# --------------------------------------------------------------------------
# 2. the literal table (the key rule's rows among them) through the engine
# --------------------------------------------------------------------------
@pytest.mark.parametrize("encap", [True, False], ids=["encap", "noencap"])
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
@pytest.mark.parametrize("mode", [LXC, NETDEV], ids=["lxc", "netdev"])
def test_literal_table(torch_cuda, mode, v6, encap):
    rows = [c for c in CASES if (c[1], c[2], c[3]) == (mode, v6, encap)]
    assert rows
    w = literal_world(encap)
    e = _engine(**engine_cfg(w))
    load_world(e, w)
    e.commit()
    cols = [case_columns(c) for c in rows]
    b = {k: np.concatenate([c[k] for c in cols]) for k in cols[0]}
    got = _run(torch_cuda, e, w, mode, v6, b)
    for i, c in enumerate(rows):
        assert tuple(int(got[k][i]) for k in COLS) == tuple(x & 0xFFFFFFFF if j > 1 else x
                                                            for j, x in enumerate(c[9])), c[0]
    e.close()


def test_key_rule(torch_cuda):
    """map keys no program builds never match: endpoint keys with a pad byte or
    the other family's tag, tunnel keys with a pad byte, a v6 tunnel key with
    p4 != 0 -- each next to a well-formed key that does"""
    w = World(host_ifindex=3, encap_ifindex=4)
    for pads in (dict(pad4=1), dict(pad5=1), dict(pad5=0x8000), dict(family=2), dict(family=0),
                 dict(pad_words=(1, 0, 0)), dict(pad_words=(0, 0, 1))):
        w.eps[key4(ip4("10.1.0.5"), **pads)] = (9, 9, 0)
        w.tun[key4(ip4("10.2.0.0"), **pads)] = key4(ip4("192.168.9.9"))
    for pads in (dict(pad4=1), dict(pad5=1), dict(family=1), dict(family=3)):
        w.eps[key6(ip6("fd00::5"), **pads)] = (9, 9, 0)
        w.tun[key6(ip6("fd01::"), **pads)] = key4(ip4("192.168.9.9"))
    w.tun[key6(ip6("fd01::1"))] = key4(ip4("192.168.9.9"))  # p4 != 0
    w.eps[key4(ip4("10.1.0.6"))] = (7, 77, 0)
    w.eps[key6(ip6("fd00::6"))] = (8, 88, 0)
    e = _engine(**engine_cfg(w))
    load_world(e, w)
    e.commit()
    b4 = dict(daddr=np.array([ip4("10.1.0.5"), ip4("10.2.3.4"), ip4("10.1.0.6")], np.uint32))
    got = _run(torch_cuda, e, w, NETDEV, False, b4)
    assert got["action"].tolist() == [6, 6, 3] and got["arg"].tolist() == [0, 0, 77]
    b6 = dict(daddr=np.frombuffer(ip6("fd00::5") + ip6("fd01::1") + ip6("fd01::9") + ip6("fd00::6"),
                                  np.uint8).reshape(4, 16).copy(),
              verdict=np.zeros(4, np.int32), flags=np.ones(4, np.uint8))
    got = _run(torch_cuda, e, w, LXC, True, b6)
    assert got["action"].tolist() == [6, 6, 6, 3] and got["arg"].tolist() == [0, 0, 0, 88]
    # the well-formed twins match
    assert e.endpoint_update(L.endpoint_key("10.1.0.5"), 0, L.endpoint_info(1, 11)) == 0
    assert e.tunnel_update(L.endpoint_key("fd01::"), L.endpoint_key("192.168.0.7")) == 0
    e.commit()
    assert _run(torch_cuda, e, w, NETDEV, False, b4)["arg"].tolist() == [11, 0, 77]
    got = _run(torch_cuda, e, w, LXC, True, b6)
    assert got["action"].tolist() == [6, 5, 5, 3] and got["arg"][1] == ip4("192.168.0.7")
    e.close()


# --------------------------------------------------------------------------
# 3. tables under load
# --------------------------------------------------------------------------
def test_tables_under_load(torch_cuda):
    rng = np.random.default_rng(5)
    n_ep, n_tun = 20_000, 60_000
    low = rng.choice(2 * 65536, n_ep, replace=False).astype(np.uint32)  # two /16s: 10.1.0.0/16, 10.2.0.0/16
    host = (np.uint32(0x0A010000) + low).astype(np.uint32)              # host order
    addr = host.byteswap()                                               # as stored
    e = _engine(endpoints_max=32768, ipv4_cluster_mask=0, ipv4_cluster_range=0)
    keys = np.zeros(n_ep, L.ENDPOINT_KEY)
    keys["ip"][:, :4] = addr.view(np.uint8).reshape(n_ep, 4)
    keys["family"] = 1
    infos = np.zeros(n_ep, L.ENDPOINT_INFO)
    infos["ifindex"] = np.arange(n_ep) + 10
    infos["lxc_id"] = (np.arange(n_ep) * 3 + 1) & 0xFFFF
    up = e.L.cgpu_endpoint_update_info
    for i in range(n_ep):
        assert up(e.h, keys[i].tobytes(), infos[i].tobytes(), 0) == 0
    pfx = rng.choice(65536, n_tun, replace=False).astype(np.uint32)      # the first two address bytes
    tk = np.zeros(n_tun, L.ENDPOINT_KEY)
    tk["ip"][:, :2] = pfx.astype("<u2").view(np.uint8).reshape(n_tun, 2)
    tk["family"] = 1
    tv = np.zeros(n_tun, L.ENDPOINT_KEY)
    tv["ip"][:, :4] = (np.arange(n_tun, dtype=np.uint32) + 1).view(np.uint8).reshape(n_tun, 4)
    tv["family"] = 1
    tup = e.L.cgpu_tunnel_update
    for i in range(n_tun):
        assert tup(e.h, tk[i].tobytes(), tv[i].tobytes(), 0) == 0
    e.commit()
    w = World()
    # every endpoint returns its own value
    got = _run(torch_cuda, e, w, NETDEV, False, dict(daddr=addr))
    assert (got["action"] == 3).all()
    np.testing.assert_array_equal(got["ifindex"], infos["ifindex"])
    np.testing.assert_array_equal(got["arg"], infos["lxc_id"])
    # the addresses +-1 around a sample, where they are no endpoints, are none
    near = np.concatenate([host[:3000] + 1, host[:3000] - 1]).astype(np.uint32)
    near = near[~np.isin(near, host)]
    assert len(near) > 3000
    exp_pfx = dict(zip(pfx.tolist(), (np.arange(n_tun) + 1).tolist()))
    nb = near.byteswap()
    got = _run(torch_cuda, e, w, NETDEV, False, dict(daddr=nb))
    want = np.array([exp_pfx.get(int(x) & 0xFFFF, 0) for x in nb], np.uint32)
    assert (got["action"] != 3).all()
    np.testing.assert_array_equal(got["action"], np.where(want != 0, 5, 6))
    np.testing.assert_array_equal(got["arg"], want)
    # every prefix answers with its own value, the 5,536 absent ones with none
    allp = np.arange(65536, dtype=np.uint32) | np.uint32(0x01020000)
    allp = allp[~np.isin(allp, addr)]
    got = _run(torch_cuda, e, w, NETDEV, False, dict(daddr=allp))
    want = np.array([exp_pfx.get(int(x) & 0xFFFF, 0) for x in allp], np.uint32)
    np.testing.assert_array_equal(got["arg"], want)
    np.testing.assert_array_equal(got["action"], np.where(want != 0, 5, 6))
    fb = e.forward_table_bytes()  # at most 50 % load, and no runaway doubling
    assert 2 * n_ep * 16 <= fb["endpoints4"] <= 16 * n_ep * 16 and 2 * n_tun * 16 <= fb["tunnel4"] <= 16 * n_tun * 16
    e.close()


def test_tables_under_load_v6(torch_cuda):
    rng = np.random.default_rng(6)
    n = 4000
    a = np.zeros((n, 16), np.uint8)
    a[:, 0] = 0xFD
    a[:, 12:] = rng.choice(1 << 20, n, replace=False).astype(">u4").view(np.uint8).reshape(n, 4)
    p = np.zeros((n, 16), np.uint8)
    p[:, 0] = 0xFC
    p[:, 8:12] = np.arange(n, dtype=">u4").view(np.uint8).reshape(n, 4)
    w = World()
    for i in range(n):
        w.eps[key6(a[i].tobytes())] = (i + 1, i & 0xFFFF, 0)
        w.tun[key6(p[i].tobytes())] = key4(i + 7)
    e = _engine(**engine_cfg(w))
    load_world(e, w)
    e.commit()
    near = a.copy()
    near[:, 15] ^= 1
    q = p.copy()
    q[:, 12:] = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    d = np.concatenate([a, near, q])
    b = dict(daddr=d, verdict=np.zeros(len(d), np.int32), flags=np.ones(len(d), np.uint8))
    exp = restate(w, LXC, True, **b)
    assert (exp["action"][:n] == 3).all() and (exp["action"][2 * n:] == 5).all() and (exp["action"][n:2 * n] == 6).any()
    _same(_run(torch_cuda, e, w, LXC, True, b), exp, "v6 load")
    e.close()


# --------------------------------------------------------------------------
# 4. alignment and NULL columns
# --------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 4], ids=["aligned", "byte", "word"])
def test_v6_daddr_alignment(torch_cuda, batch_engine, offset):
    w = batch_world()
    b = build_batch(w, True, 1029, seed=21)
    _same(_run(torch_cuda, batch_engine, w, LXC, True, b, offset=offset), restate(w, LXC, True, **b),
          f"offset {offset}")


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_null_columns(torch_cuda, batch_engine, v6):
    torch = torch_cuda
    w = batch_world()
    full = build_batch(w, v6, 777, seed=33)
    for drop in (("ttl",), ("tunnel",), ("ttl", "tunnel")):
        b = {k: (None if k in drop else x) for k, x in full.items()}
        _same(_run(torch, batch_engine, w, LXC, v6, b), restate(w, LXC, v6, **b), f"no {drop}")
    nd = {"daddr": full["daddr"], "tunnel": full["tunnel"], "ttl": full["ttl"]}  # NETDEV: no verdict, no flags
    _same(_run(torch, batch_engine, w, NETDEV, v6, nd), restate(w, NETDEV, v6, **nd), "netdev nulls")
    exp = restate(w, LXC, v6, **full)
    for keep in (("action",), ("action", "ret"), ("action", "ifindex"), ("action", "arg")):
        out = {"action": torch.empty(777, dtype=torch.uint8, device="cuda")}
        for k in COLS[1:]:
            out[k] = torch.empty(777, dtype=torch.int32, device="cuda") if k in keep else None
        got = _run(torch, batch_engine, w, LXC, v6, full, out=out)
        assert [k for k in COLS if got[k] is not None] == list(keep)
        _same(got, exp, f"outputs {keep}")
    from cilium_amd._abi import CgpuError
    with pytest.raises(CgpuError):  # LXC mode needs verdict and flags
        _run(torch, batch_engine, w, LXC, v6, nd)


# --------------------------------------------------------------------------
# 5. epochs
# --------------------------------------------------------------------------
def test_changes_are_visible_after_commit_only(torch_cuda):
    w = World(host_ifindex=3, encap_ifindex=4)
    w.eps[key4(ip4("10.1.0.5"))] = (7, 70, 0)
    w.tun[key4(ip4("10.1.0.0"))] = key4(ip4("192.168.0.2"))
    e = _engine(**engine_cfg(w))
    load_world(e, w)
    e.commit()
    b = dict(daddr=np.array([ip4("10.1.0.5"), ip4("10.2.0.5")], np.uint32),
             verdict=np.zeros(2, np.int32), flags=np.ones(2, np.uint8))
    k5 = L.endpoint_key("10.1.0.5")

    def step(change):
        before = restate(w, LXC, False, **b)
        change()
        _same(_run(torch_cuda, e, w, LXC, False, b), before, "before commit")
        e.commit()
        after = restate(w, LXC, False, **b)
        assert any((after[k] != before[k]).any() for k in COLS)
        _same(_run(torch_cuda, e, w, LXC, False, b), after, "after commit")
        return after

    def info():  # an info change
        w.eps[key4(ip4("10.1.0.5"))] = (8, 80, 0)
        assert e.endpoint_update(k5, 0, L.endpoint_info(8, 80)) == 0
    assert step(info)["arg"].tolist() == [80, 0]

    def host():  # ... to the host flag
        w.eps[key4(ip4("10.1.0.5"))] = (0, 0, ENDPOINT_F_HOST)
        assert e.endpoint_update(k5, 0, L.endpoint_info(flags=L.ENDPOINT_F_HOST)) == 0
    assert step(host)["action"].tolist() == [4, 6]

    def delete():  # the packet falls through to the tunnel map
        del w.eps[key4(ip4("10.1.0.5"))]
        assert e.endpoint_delete(k5) == 0
    assert step(delete)["action"].tolist() == [5, 6]

    def tunnel():
        w.tun[key4(ip4("10.2.0.0"))] = key4(ip4("192.168.0.3"))
        assert e.tunnel_update(L.endpoint_key("10.2.0.0"), L.endpoint_key("192.168.0.3")) == 0
    assert step(tunnel)["arg"].tolist() == [ip4("192.168.0.2"), ip4("192.168.0.3")]

    def empty():  # both maps' forwarding content gone: the tables go away, the answers stay right
        w.tun.clear()
        assert e.tunnel_delete(L.endpoint_key("10.1.0.0")) == 0 and e.tunnel_delete(L.endpoint_key("10.2.0.0")) == 0
    assert step(empty)["action"].tolist() == [6, 6]
    assert sum(e.forward_table_bytes().values()) == 0
    e.close()


@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_context_without_values_still_answers(torch_cuda, v6):
    """all infos zero, tunnel map empty (no forwarding tables are built): LOCAL
    with zeros, STACK"""
    w = World(host_ifindex=3, encap_ifindex=4)
    e = _engine(**engine_cfg(w))
    ips = [f"fd00::{i + 1:x}" for i in range(300)] if v6 else [f"10.1.{i // 250}.{i % 250 + 1}" for i in range(300)]
    for ip in ips:
        assert e.endpoint_update(L.endpoint_key(ip)) == 0
        w.eps[key6(ip6(ip)) if v6 else key4(ip4(ip))] = (0, 0, 0)
    e.commit()
    tb = e.table_bytes()
    assert sum(e.forward_table_bytes().values()) == 0
    d = [ip6(x) for x in ips] + [ip6(f"fd00::1:{i:x}") for i in range(300)] if v6 else \
        [ip4(x) for x in ips] + [ip4(f"10.2.0.{i % 250 + 1}") for i in range(300)]
    daddr = np.frombuffer(b"".join(d), np.uint8).reshape(-1, 16).copy() if v6 else np.array(d, np.uint32)
    n = len(daddr)
    b = dict(daddr=daddr, verdict=np.zeros(n, np.int32), flags=np.ones(n, np.uint8),
             tunnel=np.zeros(n, np.uint32), ttl=np.where(np.arange(n) % 7 == 0, 1, 64).astype(np.uint8))
    for mode in (LXC, NETDEV):
        exp = restate(w, mode, v6, **b)
        assert set(exp["action"][np.arange(n) % 7 != 0].tolist()) == {3, 6}
        assert (exp["ifindex"] == 0).all() and (exp["arg"] == 0).all()
        _same(_run(torch_cuda, e, w, mode, v6, b), exp, f"mode {mode}")
    # the first value builds the tables; what the other tables take is unmoved
    k = L.endpoint_key(ips[0])
    assert e.endpoint_update(k, 0, L.endpoint_info(5, 55)) == 0
    w.eps[key6(ip6(ips[0])) if v6 else key4(ip4(ips[0]))] = (5, 55, 0)
    e.commit()
    assert e.table_bytes() == tb and min(e.forward_table_bytes().values()) > 0
    _same(_run(torch_cuda, e, w, LXC, v6, b), restate(w, LXC, v6, **b), "first value")
    e.close()


# --------------------------------------------------------------------------
# 6. forward= on the classify calls
# --------------------------------------------------------------------------
FWD = dict(mode=LXC, encap=True, ipv4_mask=0xFFFF, host_ifindex=5, encap_ifindex=6)


def _cls_cols(out):
    return {k: out[k].cpu().numpy() for k in ("verdict", "identity", "stage", "tunnel", "ct_ret") if out.get(k) is not None}


def _allowed(tn, out):
    """destinations of the batch's allowed egress packets: the ones the lookups see"""
    m = ((tn["flags"] & 1) == 1) & (out["verdict"].cpu().numpy() == 0)
    u = np.unique(tn["daddr"][m], axis=0)
    assert len(u) >= 30, "the workload allows too little to compose anything"
    return u


def _fwd_load(e, u, v6):
    """a third of those destinations as endpoints (some the host's), the prefixes
    of another third in the tunnel map"""
    k = len(u) // 3
    for i, a in enumerate(u[:k]):
        raw = (a.tobytes() if v6 else int(a).to_bytes(4, "little") + bytes(12)) + bytes([2 if v6 else 1, 0, 0, 0])
        info = L.endpoint_info(i + 1, i + 100, L.ENDPOINT_F_HOST if i % 9 == 0 else 0)
        assert e.endpoint_update(np.frombuffer(raw, L.ENDPOINT_KEY)[0], 0, info) == 0
    for i, a in enumerate(u[k:2 * k]):
        raw = (a.tobytes()[:12] + bytes(4) if v6 else (int(a) & 0xFFFF).to_bytes(4, "little") + bytes(12)) + \
            bytes([2 if v6 else 1, 0, 0, 0])
        assert e.tunnel_update(np.frombuffer(raw, L.ENDPOINT_KEY)[0], L.endpoint_key(f"192.168.4.{i % 250 + 1}")) == 0


def _check_composed(torch, t, plain, tun_call, fwd_call, forward_fn):
    """fwd_call's outputs == tun_call's, then forward_fn on them; both == plain
    where plain has the column"""
    n = t["flags"].numel()
    t["ttl"] = torch.from_numpy(np.where(np.arange(n) % 5 == 0, 1, 64).astype(np.uint8)).cuda()
    sep = tun_call(t)
    f = forward_fn(t["daddr"], verdict=sep["verdict"], tunnel=sep["tunnel"], flags=t["flags"], ttl=t["ttl"], **FWD)
    got = fwd_call(t)
    torch.cuda.synchronize()
    a, b = _cls_cols(got), _cls_cols(sep)
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in COLS:
        np.testing.assert_array_equal(got["fwd_" + k].cpu().numpy(), f[k].cpu().numpy(), err_msg=k)
    if plain is not None:
        p = _cls_cols(plain(t))
        for k in p:
            np.testing.assert_array_equal(a[k], p[k], err_msg=f"plain {k}")
    acts = set(f["action"].cpu().numpy().tolist())
    return acts


def test_composition_v4(torch_cuda):
    T = synth.make_tables(n_prefixes=2000, n_identities=100, n_endpoints=2, keys_per_ep=500)
    tn = synth.make_tuples(T, 5000)
    e = _engine(**T.engine_config(), ipcache_tunnel=1)
    synth.load_engine(e, T)
    e.commit()
    t = synth.to_device(tn)
    _fwd_load(e, _allowed(tn, e.classify_v4(t)), False)
    e.commit()
    acts = _check_composed(torch_cuda, t, lambda t: e.classify_v4(t), lambda t: e.classify_v4(t, tunnel=True),
                           lambda t: e.classify_v4(t, forward=FWD), e.forward_v4)
    assert {0, 1, 3, 4, 5} <= acts, acts
    with pytest.raises(ValueError):
        e.classify_v4_lb(t, forward=FWD)
    with pytest.raises(ValueError):
        e.classify_v4_cascade(t, forward=FWD)
    with pytest.raises(TypeError):
        e.classify_v4(t, forward=dict(ttl=1))
    e.close()


def test_composition_v4_ct(torch_cuda):
    T = synth.make_tables(n_prefixes=2000, n_identities=100, n_endpoints=1, keys_per_ep=500)
    tn, locals_be, seclabels = synth.make_ct_workload(T, 400)
    es = []
    t = synth.to_device(tn)
    for _ in range(4):  # the calls change the conntrack map: one context each
        e = _engine(**T.engine_config(), ipcache_tunnel=1, ct_max=1 << 14)
        synth.load_engine(e, T)
        synth.load_lxc(e, seclabels)
        e.commit()
        es.append(e)
    u = _allowed(tn, es[3].classify_v4_ct(t, 1000))
    for e in es[:3]:
        _fwd_load(e, u, False)
        e.commit()
    acts = _check_composed(torch_cuda, t, lambda t: es[0].classify_v4_ct(t, 1000),
                           lambda t: es[1].classify_v4_ct(t, 1000, tunnel=True),
                           lambda t: es[2].classify_v4_ct(t, 1000, forward=FWD), es[1].forward_v4)
    assert {0, 3, 5} <= acts, acts
    with pytest.raises(ValueError):
        es[0].classify_v4_ctlb(t, 1000, forward=FWD)
    for e in es:
        e.close()


def test_composition_v6(torch_cuda):
    T = synth.make_tables6(n_prefixes=2000, n_identities=100, n_endpoints=2, keys_per_ep=500)
    tn = synth.make_tuples6(T, 5000)
    e = _engine(**T.engine_config(), ipcache_tunnel=1)
    synth.load_engine(e, T)
    e.commit()
    t = synth.to_device(tn)
    _fwd_load(e, _allowed(tn, e.classify_v6(t)), True)
    e.commit()
    acts = _check_composed(torch_cuda, t, lambda t: e.classify_v6(t), lambda t: e.classify_v6(t, tunnel=True),
                           lambda t: e.classify_v6(t, forward=FWD), e.forward_v6)
    assert {0, 1, 3, 4, 5} <= acts, acts
    with pytest.raises(ValueError):
        e.classify_v6_lb(t, forward=FWD)
    e.close()


def test_composition_v6_ct(torch_cuda):
    T = synth.make_tables6(n_prefixes=2000, n_identities=100, n_endpoints=1, keys_per_ep=500)
    tn, loc, seclabels = synth.make_ct6_workload(T, 400)
    es = []
    t = synth.to_device(tn)
    for _ in range(4):
        e = _engine(**T.engine_config(), ipcache_tunnel=1, ct6_max=1 << 14)
        synth.load_engine(e, T)
        synth.load_lxc(e, seclabels)
        e.commit()
        es.append(e)
    u = _allowed(tn, es[3].classify_v6_ct(t, 1000))
    for e in es[:3]:
        _fwd_load(e, u, True)
        e.commit()
    acts = _check_composed(torch_cuda, t, lambda t: es[0].classify_v6_ct(t, 1000),
                           lambda t: es[1].classify_v6_ct(t, 1000, tunnel=True),
                           lambda t: es[2].classify_v6_ct(t, 1000, forward=FWD), es[1].forward_v6)
    assert {0, 3, 5} <= acts, acts
    with pytest.raises(ValueError):
        es[0].classify_v6_ctlb(t, 1000, forward=FWD)
    for e in es:
        e.close()

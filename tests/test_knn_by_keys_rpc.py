"""GPU tests of MultiNearestNeighbor's batched by-key lookups: the by-key requests of one (space, num) in a stream window
go to the engine as ONE call (EngineSpace.nearest_many_by_key -> ehx_knn_by_keys_keys); a store without that method — the
oracle-backed one — is asked key by key and must answer the same stream the same way."""
import uuid

import grpc
import numpy as np
import pytest

from embeddinghub_amd.rpc import embedding_store_pb2 as pb
from embeddinghub_amd.rpc import server as srv
from embeddinghub_amd.rpc.client import EmbeddingHubClient
from oracle import pyoracle
from oracle.oracle_store import OracleStore

pytestmark = pytest.mark.gpu

ehx = pytest.importorskip("embeddinghub_amd")


def _serve(store):
    server, port = srv.make_server(store, "127.0.0.1:0", max_workers=8)
    server.start()
    return server, EmbeddingHubClient(host="127.0.0.1", port=port)


def _fill(c, n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    space = "byk-rpc-%s" % uuid.uuid4()
    c.create_space(space, d)
    for i in range(n):               # one Set at a time: the oracle's insertion order, and the graph engine's
        c.set(space, "k%d" % i, X[i].tolist())
    return space, X


def _mixed(space, X, Q, num):
    reqs = []
    for i in range(60):
        reqs.append(pb.NearestNeighborRequest(space=space, num=num, key="k%d" % ((i * 37) % X.shape[0])))
        if i % 3 == 0:
            reqs.append(pb.NearestNeighborRequest(space=space, num=num, embedding=pb.Embedding(values=Q[i // 3].tolist())))
        if i % 10 == 0:              # another num, a repeated key
            reqs.append(pb.NearestNeighborRequest(space=space, num=num + 2, key="k5"))
    return reqs


def test_mixed_stream_engine_store_and_oracle_store_answer_the_same():
    """the engine in graph mode, one row per insertion round, builds the oracle's graph: the key lists of one mixed stream
    are identical, whichever store answers"""
    n, d, num = 400, 12, 5
    Q = np.random.default_rng(1).standard_normal((20, d)).astype(np.float32)
    got = []
    for store in (srv.EngineStore(mode=ehx.MODE_GRAPH, build_batch=1), OracleStore()):
        server, c = _serve(store)
        try:
            space, X = _fill(c, n, d, 8)
            got.append([list(r.keys) for r in c._stub.MultiNearestNeighbor(iter(_mixed(space, X, Q, num)))])
            unary = [list(c.nearest_neighbor(space, num, key="k%d" % i)) for i in (0, 37, 74)]
            assert c.multi_nearest_neighbor(space, num, keys=["k0", "k37", "k74"]) == unary
        finally:
            c.close()
            server.stop(0)
    assert len(got[0]) == len(_mixed("s", X, Q, num)) and got[0] == got[1]


def test_flat_engine_store_by_key_stream_is_the_exhaustive_oracles():
    n, d, num = 3000, 24, 6
    server, c = _serve(srv.EngineStore())
    try:
        rng = np.random.default_rng(5)
        X = rng.standard_normal((n, d)).astype(np.float32)
        space = "byk-rpc-%s" % uuid.uuid4()
        c.create_space(space, d)
        c.multiset(space, (("k%d" % i, X[i].tolist()) for i in range(n)))
        idx = [int(i) for i in rng.integers(0, n, size=300)] + [7, 7]
        oids, _, ocnt = pyoracle.exhaustive(X, X[idx], num + 1, pyoracle.METRIC_L2)
        want = []
        for row, own in enumerate(idx):
            ids = [int(j) for j in oids[row, :int(ocnt[row])]]
            ids.pop(ids.index(own) if own in ids else len(ids) - 1)
            want.append(["k%d" % j for j in ids[:num]])
        assert c.multi_nearest_neighbor(space, num, keys=["k%d" % i for i in idx]) == want
    finally:
        c.close()
        server.stop(0)


def test_unknown_key_in_the_middle_answers_what_came_before_then_not_found():
    for store in (srv.EngineStore(), OracleStore()):
        server, c = _serve(store)
        try:
            space, X = _fill(c, 120, 8, 3)
            keys = ["k%d" % i for i in range(40)]
            want = c.multi_nearest_neighbor(space, 4, keys=keys)
            emb = pb.NearestNeighborRequest(space=space, num=4, embedding=pb.Embedding(values=X[3].tolist()))
            want_emb = list(c.nearest_neighbor(space, 4, embedding=X[3].tolist()))
            reqs = [pb.NearestNeighborRequest(space=space, num=4, key=k) for k in keys[:25]] + [emb]
            reqs += [pb.NearestNeighborRequest(space=space, num=4, key="no such key"), emb]
            reqs += [pb.NearestNeighborRequest(space=space, num=4, key=k) for k in keys[25:]]
            before = []
            with pytest.raises(grpc.RpcError) as e:
                for r in c._stub.MultiNearestNeighbor(iter(reqs)):
                    before.append(list(r.keys))
            assert e.value.code() == grpc.StatusCode.NOT_FOUND and e.value.details() == "Not found"
            assert before == want[:25] + [want_emb]
            # the unknown key first: nothing is answered
            with pytest.raises(grpc.RpcError) as e:
                list(c._stub.MultiNearestNeighbor(iter(reqs[26:])))
            assert e.value.code() == grpc.StatusCode.NOT_FOUND
        finally:
            c.close()
            server.stop(0)


def test_by_key_requests_go_through_batched_engine_calls(monkeypatch):
    calls = {"many": [], "single": 0}
    real_many, real_nearest = srv.EngineSpace.nearest_many_by_key, srv.EngineSpace.nearest

    def many(self, num, keys):
        calls["many"].append(len(keys))
        return real_many(self, num, keys)

    def nearest(self, num, key="", embedding=None):
        if key != "":
            calls["single"] += 1
        return real_nearest(self, num, key=key, embedding=embedding)
    monkeypatch.setattr(srv.EngineSpace, "nearest_many_by_key", many)
    monkeypatch.setattr(srv.EngineSpace, "nearest", nearest)
    server_store = srv.EngineStore()
    server, c = _serve(server_store)
    try:
        space, X = _fill(c, 200, 8, 4)
        keys = ["k%d" % (i % 200) for i in range(500)]
        got = c.multi_nearest_neighbor(space, 3, keys=keys)
        assert len(got) == 500 and got[:200] == got[200:400]
        # the stream is cut into windows as it arrives (a window with ONE by-key request asks for it alone): every request
        # was answered by exactly one engine call, and requests that shared a window shared a batched call
        assert sum(calls["many"]) + calls["single"] == 500
        assert calls["many"] and max(calls["many"]) > 1
        print("batched calls:", calls["many"], "single calls:", calls["single"])
        # ... and without the stream's timing: the by-key requests of one window group are ONE engine call (a second one,
        # for the keys in front of it, when a key is unknown), never a call per key
        sp = server_store.get_space(space)
        calls["many"], calls["single"] = [], 0
        got1, bad = srv.EmbeddingHubService._nearest_by_keys(sp, 3, keys[:300])
        assert bad is None and got1 == got[:300] and calls == {"many": [300], "single": 0}
        calls["many"] = []
        got2, bad = srv.EmbeddingHubService._nearest_by_keys(sp, 3, keys[:40] + ["no such key"] + keys[40:80])
        assert bad == 40 and got2 == got[:40] and calls == {"many": [81, 40], "single": 0}
    finally:
        c.close()
        server.stop(0)

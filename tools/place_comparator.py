"""The CPU comparator of tools/next_tier_bench.py's place-recognition row: KeyFrameDatabase's two candidate queries
(thirdparty/orb-slam2/src/KeyFrameDatabase.cc:53-59, 89-310, with L1Scoring::score, ScoringObject.cpp:23-60) restated in plain
C++ on std::map BowVectors and std::list inverted lists, one core.  The source below is compiled with g++ on first use into a
temporary directory and called through ctypes.  It is a restatement written for this tool -- NOT ORB-SLAM2 -- and is held equal to
tests/place_reference.py on the constructed cases by tests/test_place_comparator.py.

place_cpu runs nq queries over one table in the layout of pgorb_detect_*_candidates (CSR BowVectors, membership in add order,
neighbour CSR); like the batched device forms, every query starts from the same stored scores.  *seconds = the queries alone
(the database is built before the clock starts)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

SOURCE = r"""
#include <chrono>
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <vector>

struct KeyFrame {
    int row;
    std::map<uint32_t, double> bow;                        // DBoW2::BowVector
    std::vector<KeyFrame*> ordered;                        // mvpOrderedConnectedKeyFrames
    long relocQuery = -1, loopQuery = -1;
    int relocWords = 0, loopWords = 0;
    float relocScore = 0.f, loopScore = 0.f;
    bool scored = false;
};

static double score_l1(const std::map<uint32_t, double>& v1, const std::map<uint32_t, double>& v2)
{
    auto i1 = v1.begin(), i2 = v2.begin();
    double score = 0;
    while (i1 != v1.end() && i2 != v2.end()) {
        if (i1->first == i2->first) { score += std::fabs(i1->second - i2->second) - std::fabs(i1->second) - std::fabs(i2->second); ++i1; ++i2; }
        else if (i1->first < i2->first) i1 = v1.lower_bound(i2->first);
        else i2 = v2.lower_bound(i1->first);
    }
    return -score / 2.0;
}

extern "C" int place_cpu(int loop, int nkf, const int* bow_start, const uint32_t* bow_id, const double* bow_val, const uint8_t* in_db,
                         const int* neigh_start, const int* neigh, const int* queries, int nq, const float* state, const float* min_score,
                         const int* conn_start, const int* conn, int* cand, int ccap, int* ncand, int* common, float* score, int* stats,
                         double* seconds)
{
    std::vector<KeyFrame> kfs(nkf);
    std::map<uint32_t, std::list<KeyFrame*>> inverted;     // mvInvertedFile
    for (int f = 0; f < nkf; f++) {
        kfs[f].row = f;
        for (int k = bow_start[f]; k < bow_start[f + 1]; k++) kfs[f].bow[bow_id[k]] = bow_val[k];
        for (int k = neigh_start[f]; k < neigh_start[f + 1]; k++) kfs[f].ordered.push_back(&kfs[neigh[k]]);
    }
    for (int f = 0; f < nkf; f++)                         // add(), in table order
        if (in_db[f]) for (auto& wv : kfs[f].bow) inverted[wv.first].push_back(&kfs[f]);
    const auto t0 = std::chrono::steady_clock::now();
    for (int q = 0; q < nq; q++) {
        KeyFrame& Q = kfs[queries[q]];
        const long id = 1000000 + q;
        for (int f = 0; f < nkf; f++) { kfs[f].relocScore = state ? state[f] : 0.f; kfs[f].loopScore = 0.f; kfs[f].scored = false; }
        std::set<KeyFrame*> connected;
        if (loop) for (int k = conn_start[q]; k < conn_start[q + 1]; k++) connected.insert(&kfs[conn[k]]);
        std::list<KeyFrame*> sharing;
        for (auto& wv : Q.bow) {
            auto it = inverted.find(wv.first);
            if (it == inverted.end()) continue;
            for (KeyFrame* k : it->second) {
                if (loop) {
                    if (k->loopQuery != id) { k->loopWords = 0; if (!connected.count(k)) { k->loopQuery = id; sharing.push_back(k); } }
                    k->loopWords++;
                } else {
                    if (k->relocQuery != id) { k->relocWords = 0; k->relocQuery = id; sharing.push_back(k); }
                    k->relocWords++;
                }
            }
        }
        int* com = common + (long)q * nkf;
        float* sc = score + (long)q * nkf;
        for (int f = 0; f < nkf; f++) com[f] = 0;
        int maxCommon = 0, nscores = 0;
        for (KeyFrame* k : sharing) { const int w = loop ? k->loopWords : k->relocWords; com[k->row] = w; if (w > maxCommon) maxCommon = w; }
        int minCommon = maxCommon * 0.8f;
        std::list<std::pair<float, KeyFrame*>> scoreAndMatch, accAndMatch;
        const float minScore = loop ? min_score[q] : 0.f;
        for (KeyFrame* k : sharing) {
            if ((loop ? k->loopWords : k->relocWords) > minCommon) {
                nscores++;
                float si = score_l1(Q.bow, k->bow);
                if (loop) { k->loopScore = si; if (si >= minScore) scoreAndMatch.push_back({si, k}); }
                else { k->relocScore = si; scoreAndMatch.push_back({si, k}); }
            }
        }
        float bestAcc = minScore;
        for (auto& e : scoreAndMatch) {
            KeyFrame* k = e.second;
            float bestScore = e.first, acc = e.first;
            KeyFrame* best = k;
            int taken = 0;
            for (KeyFrame* k2 : k->ordered) {
                if (taken++ == 10) break;
                if (loop) { if (!(k2->loopQuery == id && k2->loopWords > minCommon)) continue; }
                else if (k2->relocQuery != id) continue;
                const float v = loop ? k2->loopScore : k2->relocScore;
                acc += v;
                if (v > bestScore) { best = k2; bestScore = v; }
            }
            accAndMatch.push_back({acc, best});
            if (acc > bestAcc) bestAcc = acc;
        }
        const float keep = 0.75f * bestAcc;
        std::set<KeyFrame*> already;
        int n = 0;
        for (auto& e : accAndMatch)
            if (e.first > keep && !already.count(e.second)) {
                if (n < ccap) cand[(long)q * ccap + n] = e.second->row;
                n++;
                already.insert(e.second);
            }
        ncand[q] = n;
        for (int f = 0; f < nkf; f++) sc[f] = loop ? kfs[f].loopScore : kfs[f].relocScore;
        stats[3 * q] = (int)sharing.size(); stats[3 * q + 1] = maxCommon; stats[3 * q + 2] = nscores;
    }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
"""

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="place_cpu_")
        src, so = os.path.join(_dir.name, "place_cpu.cc"), os.path.join(_dir.name, "place_cpu.so")
        with open(src, "w") as f:
            f.write(SOURCE)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
        _lib = C.CDLL(so)
        _lib.place_cpu.restype = C.c_int
        _lib.place_cpu.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5
    return _lib


def run(loop, bow_start, bow_id, bow_val, in_db, neigh_start, neigh, queries, state=None, min_score=None, conn_start=None, conn=None, ccap=64):
    """Returns (cand [nq][ccap], ncand, common [nq][nkf], score [nq][nkf], stats [nq][3], seconds of the queries)."""
    a = lambda x, dt: np.ascontiguousarray(x, dt)
    bow_start, bow_id, bow_val, in_db = a(bow_start, np.int32), a(bow_id, np.uint32), a(bow_val, np.float64), a(in_db, np.uint8)
    neigh_start, neigh, queries = a(neigh_start, np.int32), a(neigh, np.int32), a(queries, np.int32)
    nkf, nq = len(in_db), len(queries)
    state = None if state is None else a(state, np.float32)
    min_score = a(np.zeros(nq) if min_score is None else min_score, np.float32)
    conn_start = a(np.zeros(nq + 1) if conn_start is None else conn_start, np.int32)
    conn = a([] if conn is None else conn, np.int32)
    cand, ncand = np.full((nq, max(ccap, 1)), -1, np.int32), np.zeros(nq, np.int32)
    common, score, stats = np.zeros((nq, nkf), np.int32), np.zeros((nq, nkf), np.float32), np.zeros((nq, 3), np.int32)
    sec = C.c_double(0)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    rc = lib().place_cpu(int(loop), nkf, p(bow_start), p(bow_id), p(bow_val), p(in_db), p(neigh_start), p(neigh), p(queries), nq, p(state),
                         p(min_score), p(conn_start), p(conn), p(cand), ccap, p(ncand), p(common), p(score), p(stats), C.addressof(sec))
    assert rc == 0
    return cand, ncand, common, score, stats, sec.value

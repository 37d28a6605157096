// Sanitizer run of the frame producer's label pass (nvspeechplayer_amd/csrc/frame_producer.cpp) on the CPU: the symbol soup of
// fuzz_producer.cpp -- tie bars, stress and length marks anywhere, unknown symbols, invalid UTF-8 -- through speechPlayer_ipa_labels,
// speechPlayer_ipa_records + speechPlayer_records_labels and the batch entry points, under AddressSanitizer + UBSan
// (tests/test_alignment_host.py builds and runs it).  Every label is checked against the contract of include/speechPlayer_batch.h.
// The engine's entry points are stubbed: this links no GPU code.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "speechPlayer_batch.h"

static long long g_labelled = 0;
static std::vector<speechPlayer_frameLabel_t> g_lastLabels;      // what the last labelled set call was handed, and its lists
static std::vector<long long> g_lastStart;
static bool g_textOffsets = true;       // false while speechPlayer_batch_setText is checked: its labels carry no text offsets

static bool labels_ok(const speechPlayer_frameLabel_t* l, long long n, long long textBytes)
{
    const int count = speechPlayer_ipa_phonemeCount();
    int units = 0;
    for (long long k = 0; k < n; ++k) {
        if (l[k].phoneme < 0 || l[k].phoneme > count + 1) return false;
        if (l[k].unit == units) ++units; else if (l[k].unit != units - 1) return false;
        const bool inserted = (l[k].flags & (SPEECHPLAYER_LABEL_GAP | SPEECHPLAYER_LABEL_PUFF)) != 0 || l[k].phoneme == count + 1;
        if (inserted || !g_textOffsets ? l[k].textOffset != -1 : (l[k].textOffset < 0 || (textBytes >= 0 && l[k].textOffset >= textBytes))) return false;
        if ((l[k].flags & SPEECHPLAYER_LABEL_GAP) ? l[k].phoneme != count : l[k].phoneme == count) return false;
        if ((l[k].flags & SPEECHPLAYER_LABEL_STRESS_MASK) == 3 || l[k].flags >= 512u) return false;
    }
    return true;
}

extern "C" int speechPlayer_batch_sampleRate(speechPlayer_batch_t) { return 22050; }
extern "C" void speechPlayer_internal_setError(int, const char*) {}
extern "C" int speechPlayer_batch_setRecords(speechPlayer_batch_t, long long, const speechPlayer_frame_t*, long long, const long long*, const speechPlayer_frameRecord_t*,
                                             long long, const unsigned int*, const unsigned int*) { return -1; }      // (a text batch must arrive labelled)
extern "C" int speechPlayer_batch_setRecordsLabelled(speechPlayer_batch_t, long long nShapes, const speechPlayer_frame_t*, long long nLists, const long long* listStart,
                                                     const speechPlayer_frameRecord_t* rec, const speechPlayer_frameLabel_t* labels, long long nUtt,
                                                     const unsigned int* listOf, const unsigned int*)
{
    if (!labels) return -1;
    for (long long u = 0; listOf && u < nUtt; ++u) if ((long long)listOf[u] >= nLists) return -1;
    for (long long k = 0; k < listStart[nLists]; ++k) if (rec[k].shape != SPEECHPLAYER_RECORD_SILENCE && (long long)rec[k].shape >= nShapes) return -1;
    for (long long l = 0; l < nLists; ++l) {
        if (!labels_ok(labels + listStart[l], listStart[l + 1] - listStart[l], -1)) return -1;
        for (long long k = listStart[l]; k < listStart[l + 1]; ++k)
            if ((rec[k].shape == SPEECHPLAYER_RECORD_SILENCE) != (labels[k].phoneme >= speechPlayer_ipa_phonemeCount())) return -1;
        g_labelled += listStart[l + 1] - listStart[l];
    }
    g_lastLabels.assign(labels, labels + listStart[nLists]);
    g_lastStart.assign(listStart, listStart + nLists + 1);
    return 0;
}
extern "C" int speechPlayer_node_setRecords(speechPlayer_node_t, long long, const speechPlayer_frame_t*, long long, const long long*, const speechPlayer_frameRecord_t*,
                                            long long, const unsigned int*, const unsigned int*) { return 0; }
extern "C" void speechPlayer_internal_parallel(long long n, long long, void (*fn)(void*, long long, long long), void* ctx)
{
    if (n > 0) { fn(ctx, 0, n / 2); fn(ctx, n / 2, n); }
}

// speechPlayer_batch_setText over a stand-in for eSpeak that answers a clause with the clause itself (tests/native/fake_espeak.c): an
// utterance's labels are its clauses' labels one after the other with the units counting on, no text offsets, and one silence at the end.
static int check_set_text(const char* fakeEspeak)
{
    setenv("SPEECHPLAYER_ESPEAK_LIB", fakeEspeak, 1);
    if (!speechPlayer_text_available()) { printf("the stand-in for eSpeak did not load\n"); return 1; }
    const char* texts[] = {"h\xc3\xa6lou, w\xc9\x9c\xcb\x90ld. p t k", "\xcb\x88t\xcd\xa1\xca\x83\xc9\x91", "t\xc9\x91! k\xc3\xa6t; p\xc9\x91\xcb\x90: ", "#"};
    const long long nTexts = sizeof texts / sizeof *texts;
    g_lastLabels.clear(); g_lastStart.clear();
    g_textOffsets = false;
    const int rc = speechPlayer_batch_setText(nullptr, nTexts, texts, "en", 1.0, nullptr, 0.5, nullptr, nullptr);
    g_textOffsets = true;
    if (rc != 0) { printf("setText failed\n"); return 1; }
    if ((long long)g_lastStart.size() != nTexts + 1) { printf("setText: %zu lists\n", g_lastStart.size()); return 1; }
    const int count = speechPlayer_ipa_phonemeCount();
    for (long long i = 0; i < nTexts; ++i) {
        long long b[16], e[16];
        const long long nc = speechPlayer_text_clauses(texts[i], b, e, nullptr, nullptr, 16);
        std::vector<speechPlayer_frameLabel_t> want;
        int unit0 = 0;
        for (long long c = 0; c < nc; ++c) {
            const std::string clause(texts[i] + b[c], texts[i] + e[c]);
            const long long n = speechPlayer_ipa_labels(clause.c_str(), nullptr, nullptr, nullptr, nullptr, 0);
            std::vector<int> ph(n + 1), un(n + 1), off(n + 1); std::vector<unsigned> fl(n + 1);
            speechPlayer_ipa_labels(clause.c_str(), ph.data(), fl.data(), un.data(), off.data(), n);
            int units = 0;
            for (long long k = 0; k < n; ++k) { want.push_back(speechPlayer_frameLabel_t{ph[k], fl[k], unit0 + un[k], -1}); units = un[k] + 1; }
            unit0 += units;
        }
        want.push_back(speechPlayer_frameLabel_t{count + 1, 0u, unit0, -1});
        const long long a = g_lastStart[i], z = g_lastStart[i + 1];
        if (z - a != (long long)want.size()) { printf("setText: text %lld has %lld labels, %zu expected\n", i, z - a, want.size()); return 1; }
        for (long long k = 0; k < z - a; ++k) {
            const speechPlayer_frameLabel_t& g = g_lastLabels[a + k], & w = want[k];
            if (g.phoneme != w.phoneme || g.flags != w.flags || g.unit != w.unit || g.textOffset != w.textOffset) { printf("setText: text %lld label %lld\n", i, k); return 1; }
        }
        if (i == 0 && (nc != 3 || unit0 != 12)) { printf("setText: %lld clauses, %d units\n", nc, unit0); return 1; }
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && check_set_text(argv[1])) return 1;
    std::mt19937 rng(2);
    const char* alphabet[] = {"a","h","t","\xcd\xa1","\xca\x83","\xcb\x88","\xcb\x8c","\xcb\x90"," ","p","s","z","m","n","l","j","w","\xc9\x91","\xc3\xa6","i","u","#","\xff","\xc9","d","\xca\x92","k","b","\xc9\xb9","\xc5\x8b"};
    const int na = sizeof alphabet / sizeof *alphabet;
    long long total = 0;
    for (int iter = 0; iter < 40000; ++iter) {
        std::string s;
        const int len = rng() % 24;
        for (int i = 0; i < len; ++i) s += alphabet[rng() % na];
        const long long n = speechPlayer_ipa_labels(s.c_str(), nullptr, nullptr, nullptr, nullptr, 0);
        const long long frames = speechPlayer_ipa_frames(s.c_str(), 1.0, 100.0, 0.5, '.', nullptr, nullptr, nullptr, nullptr, nullptr, 0);
        if (n != frames) { printf("frame count %lld != %lld\n", n, frames); return 1; }
        if (n <= 0) continue;
        std::vector<int> ph(n), un(n), off(n); std::vector<unsigned> fl(n);
        if (speechPlayer_ipa_labels(s.c_str(), ph.data(), fl.data(), un.data(), off.data(), n) != n) { printf("mismatch\n"); return 1; }
        std::vector<speechPlayer_frameLabel_t> l(n);
        for (long long k = 0; k < n; ++k) l[k] = speechPlayer_frameLabel_t{ph[k], fl[k], un[k], off[k]};
        if (!labels_ok(l.data(), n, (long long)s.size())) { printf("bad labels for a text of %zu bytes\n", s.size()); return 1; }
        // a smaller capacity writes nothing
        int guard = -7;
        if (speechPlayer_ipa_labels(s.c_str(), &guard, nullptr, nullptr, nullptr, n - 1) != n || guard != -7) { printf("capacity\n"); return 1; }
        total += n;
    }
    // a batch with duplicates and empties: the records object's labels are parallel to its records, list by list
    std::vector<const char*> texts;
    for (int i = 0; i < 3000; ++i) texts.push_back(alphabet[i % na]);
    texts.push_back("t\xcd\xa1\xca\x83\xc9\x91 #p\xc9\x91\xcb\x90 k\xc3\xa6t");
    std::vector<int> voiceOf(texts.size());
    for (size_t i = 0; i < texts.size(); ++i) voiceOf[i] = (int)(i % 5) - 1;
    speechPlayer_records_t ro = speechPlayer_ipa_records(16000, (long long)texts.size(), texts.data(), 1.0, nullptr, 0.5, nullptr, voiceOf.data(), nullptr, 150.0);
    speechPlayer_recordsView_t view;
    const speechPlayer_frameLabel_t* labels = nullptr;
    long long nLabels = -1;
    if (!ro || speechPlayer_records_view(ro, &view) || speechPlayer_records_labels(ro, &labels, &nLabels) || nLabels != view.nRecords) { printf("records_labels\n"); return 1; }
    for (long long l = 0; l < view.nLists; ++l) {
        const long long a = view.listStart[l], e = view.listStart[l + 1];
        if (!labels_ok(labels + a, e - a, -1) || e == a || labels[e - 1].phoneme != speechPlayer_ipa_phonemeCount() + 1) { printf("list %lld\n", l); return 1; }
        for (long long k = a; k < e; ++k)
            if ((view.records[k].shape == SPEECHPLAYER_RECORD_SILENCE) != (labels[k].phoneme >= speechPlayer_ipa_phonemeCount())) { printf("record %lld\n", k); return 1; }
    }
    if (speechPlayer_records_labels(nullptr, &labels, &nLabels) != -1 || speechPlayer_records_labels(ro, nullptr, nullptr) != -1) { printf("refusals\n"); return 1; }
    speechPlayer_records_free(ro);
    if (speechPlayer_batch_setIpa(nullptr, (long long)texts.size(), texts.data(), 1.0, nullptr, 0.5, nullptr, "Benjamin", 150.0, nullptr) != 0 ||
        speechPlayer_batch_setIpaVoices(nullptr, (long long)texts.size(), texts.data(), 1.0, nullptr, 0.5, nullptr, voiceOf.data(), -1.0, nullptr) != 0) { printf("setIpa\n"); return 1; }
    printf("ok %lld labels fuzzed, %lld through the batch entry points\n", total, g_labelled);
    return g_labelled > 0 ? 0 : 1;
}

// frame_session.hip -- the frame session of the C ABI (include/dabgpu.h, "Frame session"): history ring, result slots, and the reserve /
// commit bookkeeping the receiver pipeline (receiver.hip) and the receiver bank (receiver_bank.hip) push their frames through.  Host side only.
#include <hip/hip_runtime.h>
#include <string.h>
#include <mutex>
#include <new>
#include <vector>

#include "dabgpu.h"
#include "dabgpu_internal.h"

// ------------------------------------------------------------------------------------------------
// frame session: ONE batched decode per transmission frame behind the single-stream classes
// ------------------------------------------------------------------------------------------------
// The reference fans a frame out to one FIC runner + one MSC runner per sub-channel (src/basic_radio/basic_radio.cpp:41-65), each
// calling its decoder once per FIB group / CIF: 4 + 4 x sub-channels synchronous round trips per frame behind the mirror classes.
// A session keeps the last 8 frames of soft bits on the device; push_frame copies a frame in once and launches the FIC decode and the
// time de-interleave + Viterbi of every registered sub-channel for its 4 CIFs (the batch entry points of dabgpu_decode_abi.hip, one ensemble), the
// results return to pinned host slots asynchronously, and the classes pick theirs up by (generation, group / CIF) -- see
// dab-radio_amd/host/dab/dabgpu_frame_batcher.h for when a class may use them.
// (struct dabgpu_frame_session: dabgpu_internal.h -- the receiver pipeline, receiver.hip, pushes frames that are already on the device)

// the result block: [4][96] FIB bytes | [4] FIC results | [4][n_sub] MSC results | [4][cif_out] sub-channel bytes
static size_t session_block_bytes(size_t n_sub, size_t cif_out) {
    return 4 * 96 + (4 + 4 * n_sub) * sizeof(dabgpu_codeword_result) + 4 * cif_out;
}
static void block_pointers(uint8_t* base, size_t n_sub, uint8_t** fib, dabgpu_codeword_result** fres, dabgpu_codeword_result** mres, uint8_t** msc) {
    *fib = base;
    *fres = reinterpret_cast<dabgpu_codeword_result*>(base + 4 * 96);
    *mres = *fres + 4;
    *msc = reinterpret_cast<uint8_t*>(*mres + 4 * n_sub);
}
// (re)allocates the session's device block for n_sub sub-channels of cif_out bytes per CIF; the session's stream must be idle
static int session_layout(dabgpu_frame_session* s, size_t n_sub, size_t cif_out) {
    const size_t need = session_block_bytes(n_sub, cif_out);
    if (const int st = s->d_block.regrow(need, "hipMalloc(session results)")) return st;       // (no wait here: the caller's, see above)
    block_pointers(s->d_block.get(), n_sub, &s->d_fib, &s->d_fres, &s->d_mres, &s->d_msc);
    return DABGPU_OK;
}
// the slot's pinned block for the session's current layout
static int slot_block(dabgpu_frame_session* s, dabgpu_frame_session::slot& sl) {
    const size_t need = session_block_bytes(s->subs.size(), s->cif_out);
    // (no wait: the slot's previous frame has been waited for, nothing writes the old block)
    if (const int st = sl.h_block.regrow(need, "hipHostMalloc(session results)")) return st;
    block_pointers(sl.h_block.get(), s->subs.size(), &sl.h_fib, &sl.h_fres, &sl.h_mres, &sl.h_msc);
    return DABGPU_OK;
}

extern "C" int dabgpu_frame_session_create(dabgpu_frame_session** out, int device) {
    if (!out) return DABGPU_ERR_INVALID_ARG;
    *out = nullptr;
    dabgpu_frame_session* s = new (std::nothrow) dabgpu_frame_session();
    if (!s) return DABGPU_ERR_HIP;
    int st = dabgpu_create(&s->ctx, device, nullptr, nullptr);
    if (st) { delete s; return st; }              // (no context, nothing else yet)
    st = s->d_hist.alloc((size_t)dabgpu_frame_session::H * DABGPU_NB_FRAME_BITS, "hipMalloc(session history)");
    if (!st) st = dabgpu_check_hip(hipMemsetAsync(s->d_hist.get(), 0, (size_t)dabgpu_frame_session::H * DABGPU_NB_FRAME_BITS, s->ctx->stream), "hipMemsetAsync(session history)");
    if (!st) st = dabgpu_check_hip(hipStreamSynchronize(s->ctx->stream), "hipStreamSynchronize(session history)");      // (not the NULL stream: see dabgpu_msc_stream_create)
    if (!st) st = session_layout(s, 0, 0);
    for (auto& sl : s->slots) {
        if (!st) st = slot_block(s, sl);
        if (!st) st = sl.done.create(dabgpu_wait_event_flags(false), "hipEventCreate(session)");
        if (!st) st = sl.ev_ready.create(dabgpu_wait_event_flags(false), "hipEventCreate(session)");
        if (!st) st = sl.ev_copied.create(dabgpu_wait_event_flags(false), "hipEventCreate(session)");
    }
    if (st) { dabgpu_frame_session_destroy(s); return st; }
    *out = s;
    return DABGPU_OK;
}

int dabgpu_frame_session_create_store(dabgpu_frame_session** out, dabgpu_ctx* ctx) {
    *out = nullptr;
    dabgpu_frame_session* s = new (std::nothrow) dabgpu_frame_session();
    if (!s) return DABGPU_ERR_HIP;
    s->ctx = ctx;
    s->owns_ctx = false;
    *out = s;
    return DABGPU_OK;
}

extern "C" void dabgpu_frame_session_destroy(dabgpu_frame_session* s) {
    if (!dabgpu_destroy_begin(s, s ? s->ctx : nullptr, false)) return;
    dabgpu_ctx* own = s->owns_ctx ? s->ctx : nullptr;
    if (own) (void)hipStreamSynchronize(own->stream);                   // (a store's results were waited for by the bank)
    delete s;
    if (own) dabgpu_destroy(own);
}

extern "C" int dabgpu_frame_session_set_subchannels(dabgpu_frame_session* s, const dabgpu_subchannel* subs, int n) {
    if (!s || n < 0 || n > 64 || (n && !subs)) { dabgpu_set_error("frame_session_set_subchannels: invalid argument"); return DABGPU_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lock(s->mu);
    DABGPU_BIND(s->ctx);
    std::vector<uint32_t> off((size_t)n), nb((size_t)n);
    uint32_t total = 0;
    for (int k = 0; k < n; k++) {
        int pi[4], lx[4], bytes = 0;
        if (dabgpu_subchannel_plan(&subs[k], pi, lx, &bytes) < 0 || subs[k].start_address < 0 || subs[k].start_address + subs[k].length > 864) {
            dabgpu_set_error("frame_session_set_subchannels: sub-channel %d has an invalid protection profile or exceeds 864 CU", k);
            return DABGPU_ERR_INVALID_ARG;
        }
        off[(size_t)k] = total; nb[(size_t)k] = (uint32_t)bytes; total += (uint32_t)bytes;
    }
    int st = dabgpu_check_hip(hipStreamSynchronize(s->ctx->stream), "hipStreamSynchronize(session)");
    if (st) return st;
    if ((st = session_layout(s, (size_t)n, total))) return st;
    s->subs.assign(subs, subs + n); s->sub_off = off; s->sub_n = nb; s->cif_out = total;
    return DABGPU_OK;
}

// The decode of generation `gen` on the session's stream: FIC of the frame in history slot gen % H, MSC of its 4 CIFs (the time
// de-interleaver reaches 4 frames back), results to the slot's pinned buffers, the slot's done event.  s->mu held.
static int session_decode(dabgpu_frame_session* s, uint64_t gen, dabgpu_frame_session::slot& sl, int decode_fic, int tie_rule) {
    dabgpu_ctx* c = s->ctx;
    hipStream_t q = c->stream;
    const int hs = (int)(gen % dabgpu_frame_session::H);
    int8_t* d_frame = s->d_hist.get() + (size_t)hs * DABGPU_NB_FRAME_BITS;
    const int n_sub = (int)s->subs.size();
    int st;
    sl.fic = decode_fic != 0;
    sl.subs = s->subs; sl.sub_off = s->sub_off; sl.sub_n = s->sub_n; sl.cif_out = s->cif_out;
    if ((st = slot_block(s, sl))) return st;
    if (decode_fic && !n_sub) {
        if ((st = dabgpu_fic_decode_frames(c, d_frame, 1, DABGPU_NB_FRAME_BITS, s->d_fib, s->d_fres, tie_rule, q))) return st;
    }
    if (n_sub) {
        const size_t need = (size_t)4 * s->cif_out;
        // the frame's FIC and sub-channels in one call (one launch in the wave mapping: msc_decode_any)
        if (decode_fic) st = dabgpu_decode_frames_layout(c, s->d_hist.get(), 1, (size_t)dabgpu_frame_session::H * DABGPU_NB_FRAME_BITS, dabgpu_frame_session::H, hs,
                                                         s->subs.data(), n_sub, s->d_fib, s->d_fres, s->d_msc, need, s->d_mres, tie_rule, DABGPU_BITS_NATURAL, q);
        else st = dabgpu_msc_decode_frames(c, s->d_hist.get(), 1, (size_t)dabgpu_frame_session::H * DABGPU_NB_FRAME_BITS, dabgpu_frame_session::H, hs,
                                           s->subs.data(), n_sub, s->d_msc, need, s->d_mres, tie_rule, q);
        if (st) return st;
    }
    // one copy: the whole block with sub-channels, its FIC head without
    if (n_sub || decode_fic)
        DABGPU_CK(hipMemcpyAsync(sl.h_block.get(), s->d_block.get(), n_sub ? session_block_bytes((size_t)n_sub, s->cif_out) : session_block_bytes(0, 0), hipMemcpyDeviceToHost, q));
    return DABGPU_OK;
}

extern "C" int dabgpu_frame_session_push_frame(dabgpu_frame_session* s, const int8_t* h_bits, int decode_fic, int tie_rule, uint64_t* generation) {
    if (!s || !h_bits) { dabgpu_set_error("frame_session_push_frame: null argument"); return DABGPU_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> lock(s->mu);
    dabgpu_ctx* c = s->ctx;
    DABGPU_BIND(c);
    hipStream_t q = c->stream;
    if (s->next_reserve != s->next_gen) { dabgpu_set_error("frame_session_push_frame: a reserved frame has not been committed"); return DABGPU_ERR_INVALID_ARG; }
    const uint64_t gen = s->next_gen;
    const int hs = (int)(gen % dabgpu_frame_session::H);
    dabgpu_frame_session::slot& sl = s->slots[gen % dabgpu_frame_session::R];
    int st;
    if (sl.pending) {                                                   // the slot's previous frame (R frames ago)
        if ((st = dabgpu_check_hip(hipEventSynchronize(sl.done.get()), "hipEventSynchronize(session)"))) return st;
        sl.pending = false;
    }
    int8_t* d_frame = s->d_hist.get() + (size_t)hs * DABGPU_NB_FRAME_BITS;
    if ((st = dabgpu_stage_h2d(c, d_frame, h_bits, DABGPU_NB_FRAME_BITS, q))) return st;
    sl.gen = ~0ull;
    if ((st = session_decode(s, gen, sl, decode_fic, tie_rule))) return st;
    if ((st = dabgpu_check_hip(hipEventRecord(sl.done.get(), q), "hipEventRecord(session)"))) return st;
    sl.pending = true;
    sl.gen = gen;
    s->next_gen = gen + 1;
    s->next_reserve = gen + 1;
    if (generation) *generation = gen;
    return DABGPU_OK;
}

int dabgpu_session_reserve(dabgpu_frame_session* s, hipStream_t producer, uint64_t* gen_out, int8_t** d_frame_bits, dabgpu_frame_session::slot** slot_out) {
    DABGPU_BIND(s->ctx);
    int st;
    {   // the slot's previous frame (R frames ago) is waited for OUTSIDE the session's lock: the decode thread's commit and every decoder's fetch of
        // this receiver (and, through the batcher, of the others) take that lock.  Reservations come from one thread (the header's contract),
        // so next_reserve cannot move while this one waits
        hipEvent_t done = nullptr;
        uint64_t gen0;
        {
            std::lock_guard<std::mutex> lock(s->mu);
            gen0 = s->next_reserve;
            dabgpu_frame_session::slot& sl0 = s->slots[gen0 % dabgpu_frame_session::R];
            if (sl0.pending) done = sl0.done.get();
        }
        if (done) {
            if ((st = dabgpu_check_hip(hipEventSynchronize(done), "hipEventSynchronize(session)"))) return st;
            std::lock_guard<std::mutex> lock(s->mu);
            dabgpu_frame_session::slot& sl0 = s->slots[gen0 % dabgpu_frame_session::R];
            if (s->next_reserve == gen0 && sl0.done.get() == done) sl0.pending = false;
        }
    }
    std::lock_guard<std::mutex> lock(s->mu);
    const uint64_t gen = s->next_reserve;
    // the commits (decode enqueued) may lag the reservations by a few frames (dabgpu_receiver_submit_demod / _submit_decode on two threads), but the
    // result slot and the history slot of `gen` must be free: R - 1 frames at most may be reserved and not yet waited for
    if (gen >= s->next_gen + (uint64_t)(dabgpu_frame_session::R - 1)) {
        dabgpu_set_error("session_reserve: %d frames reserved and not committed (at most %d)", (int)(gen - s->next_gen), dabgpu_frame_session::R - 1);
        return DABGPU_ERR_NOT_READY;
    }
    dabgpu_frame_session::slot& sl = s->slots[gen % dabgpu_frame_session::R];
    if (sl.pending) {                                                  // (only if the wait above raced with a commit of that slot: cannot happen with one reserving thread)
        if ((st = dabgpu_check_hip(hipEventSynchronize(sl.done.get()), "hipEventSynchronize(session)"))) return st;
        sl.pending = false;
    }
    // history slot gen % H holds frame gen - H, which the decodes of the frames gen - H .. gen - 4 read (5 frames = 16 CIFs + the frame's own
    // 4): the producer may overwrite it once the decode of frame gen - 4 has run (the decodes run in order on one stream)
    if (gen >= 4) {
        if (gen - 4 >= s->next_gen) {
            dabgpu_set_error("session_reserve: the decode of frame %llu has not been submitted, frame %llu would overwrite what it reads (at most 4 frames "
                             "between dabgpu_receiver_submit_demod and dabgpu_receiver_submit_decode)", (unsigned long long)(gen - 4), (unsigned long long)gen);
            return DABGPU_ERR_NOT_READY;
        }
        dabgpu_frame_session::slot& old = s->slots[(gen - 4) % dabgpu_frame_session::R];
        if (old.pending && old.gen == gen - 4 &&
            (st = dabgpu_check_hip(hipStreamWaitEvent(producer, old.done.get(), 0), "hipStreamWaitEvent(session history)"))) return st;
    }
    sl.gen = ~0ull;
    s->next_reserve = gen + 1;
    *gen_out = gen;
    *d_frame_bits = s->d_hist.get() + (size_t)(gen % dabgpu_frame_session::H) * DABGPU_NB_FRAME_BITS;
    *slot_out = &sl;
    return DABGPU_OK;
}

int dabgpu_session_commit(dabgpu_frame_session* s, uint64_t gen, hipEvent_t ready, size_t bits_bytes, int decode, int decode_fic, int tie_rule,
                          hipEvent_t producer_done) {
    std::lock_guard<std::mutex> lock(s->mu);
    dabgpu_ctx* c = s->ctx;
    DABGPU_BIND(c);
    if (gen != s->next_gen) { dabgpu_set_error("session_commit: generation %llu was not the one reserved", (unsigned long long)gen); return DABGPU_ERR_INVALID_ARG; }
    if (gen >= s->next_reserve) {                                       // (a decode submitted before its demodulation: the slot's ready event is stale or was never recorded)
        dabgpu_set_error("session_commit: generation %llu has not been reserved (dabgpu_receiver_submit_demod comes first)", (unsigned long long)gen);
        return DABGPU_ERR_NOT_READY;
    }
    hipStream_t q = c->stream;
    dabgpu_frame_session::slot& sl = s->slots[gen % dabgpu_frame_session::R];
    int st;
    if (ready && (st = dabgpu_check_hip(hipStreamWaitEvent(q, ready, 0), "hipStreamWaitEvent(session producer)"))) return st;
    if (bits_bytes) {
        if (!sl.h_bits && (st = sl.h_bits.alloc(DABGPU_NB_FRAME_BITS, "hipHostMalloc(session bits)"))) return st;
        if ((st = dabgpu_check_hip(hipMemcpyAsync(sl.h_bits.get(), s->d_hist.get() + (size_t)(gen % dabgpu_frame_session::H) * DABGPU_NB_FRAME_BITS, bits_bytes,
                                                  hipMemcpyDeviceToHost, q), "hipMemcpyAsync(session bits)"))) return st;
    }
    sl.fic = false; sl.subs.clear(); sl.sub_off.clear(); sl.sub_n.clear(); sl.cif_out = 0;
    if (decode && (st = session_decode(s, gen, sl, decode_fic, tie_rule))) return st;
    if (producer_done && (st = dabgpu_check_hip(hipStreamWaitEvent(q, producer_done, 0), "hipStreamWaitEvent(session producer copies)"))) return st;
    if ((st = dabgpu_check_hip(hipEventRecord(sl.done.get(), q), "hipEventRecord(session)"))) return st;
    sl.pending = true;
    sl.gen = gen;
    s->next_gen = gen + 1;
    return DABGPU_OK;
}

// a reservation whose producer failed before anything of the frame was enqueued for the decoder: give the generation back (only the NEWEST
// reservation can be returned, and only while it has not been committed)
void dabgpu_session_unreserve(dabgpu_frame_session* s, uint64_t gen) {
    std::lock_guard<std::mutex> lock(s->mu);
    if (gen + 1 == s->next_reserve && gen >= s->next_gen) s->next_reserve = gen;
}

int dabgpu_session_slot(dabgpu_frame_session* s, uint64_t gen, dabgpu_frame_session::slot** out) {
    dabgpu_frame_session::slot& sl = s->slots[gen % dabgpu_frame_session::R];
    if (sl.gen != gen) return DABGPU_ERR_NOT_READY;                     // never pushed, or overwritten by a later frame
    if (sl.pending) {
        DABGPU_BIND(s->ctx);
        int st = dabgpu_check_hip(hipEventSynchronize(sl.done.get()), "hipEventSynchronize(session)");
        if (st) return st;
        sl.pending = false;
    }
    *out = &sl;
    return DABGPU_OK;
}

extern "C" int dabgpu_frame_session_fetch_fib_group(dabgpu_frame_session* s, uint64_t generation, int group, uint8_t* h_bytes,
                                                    uint32_t* crc_ok_mask, uint64_t* path_error) {
    if (!s || group < 0 || group > 3 || !h_bytes) return DABGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(s->mu);
    dabgpu_frame_session::slot* sl = nullptr;
    int st = dabgpu_session_slot(s, generation, &sl);
    if (st) return st;
    if (!sl->fic) return DABGPU_ERR_NOT_READY;
    memcpy(h_bytes, sl->h_fib + 96 * group, 96);
    if (crc_ok_mask) *crc_ok_mask = sl->h_fres[group].crc_ok_mask;
    if (path_error) *path_error = sl->h_fres[group].path_error;
    return DABGPU_OK;
}

extern "C" int dabgpu_frame_session_fetch_cif(dabgpu_frame_session* s, uint64_t generation, const dabgpu_subchannel* sc, int cif,
                                              uint8_t* h_bytes, size_t capacity, size_t* n_bytes, uint64_t* path_error) {
    if (!s || !sc || cif < 0 || cif > 3 || !h_bytes || !n_bytes) return DABGPU_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(s->mu);
    dabgpu_frame_session::slot* sl = nullptr;
    int st = dabgpu_session_slot(s, generation, &sl);
    if (st) return st;
    for (size_t k = 0; k < sl->subs.size(); k++) {
        if (memcmp(&sl->subs[k], sc, sizeof(dabgpu_subchannel)) != 0) continue;
        if (sl->sub_n[k] > capacity) return DABGPU_ERR_INVALID_ARG;
        memcpy(h_bytes, sl->h_msc + (size_t)cif * sl->cif_out + sl->sub_off[k], sl->sub_n[k]);
        *n_bytes = sl->sub_n[k];
        if (path_error) *path_error = sl->h_mres[(size_t)cif * sl->subs.size() + k].path_error;
        return DABGPU_OK;
    }
    return DABGPU_ERR_NOT_READY;                                        // the sub-channel was not registered when that frame was pushed
}

// receiver_bank_sched.h -- the boundary between the receiver bank's two halves: receiver_bank_sched.cpp (plain C++: what happens when) and
// receiver_bank.hip (the device work of a round).  No runtime header here: the scheduler is also built under sanitizers on a machine without a GPU,
// over a CPU implementation of rx_bank_device (tests/cpp/fake_dabgpu_oracle.cpp).
#pragma once
#include <condition_variable>
#include <vector>

#include "receiver_bank.h"

constexpr int RX_BANK_TICKS = 8;                // rounds that may be under way (their buffers)
constexpr int RX_BANK_SLOTS = 8;                // result slots of a member's frame session (dabgpu_frame_session::R, dabgpu_internal.h)
constexpr int RX_BANK_UPLOADS = 3;              // upload streams (member slot % n): frames cross PCIe on several DMA engines at once
// Frames of samples a member's device half keeps: upload puts frame gen into buffer gen % RX_BANK_IQ_FRAMES, on a stream that waits for nothing.  As many
// as result slots: post_frame accepts gen only while gen < done_gen + RX_BANK_SLOTS - 1, so frame gen - RX_BANK_SLOTS has been handed out -- the completer
// waited for the device work of its round, the gather of its samples included, before this upload could be enqueued.  (Two buffers were not enough: up to
// RX_BANK_SLOTS - 1 frames may be posted with no synchroniser in between, and the third overwrote the first before its round had read it.)
constexpr int RX_BANK_IQ_FRAMES = RX_BANK_SLOTS;

struct rx_member_device;                        // the device half of a member: whatever the rx_bank_device in use keeps per member

struct rx_bank_job {
    enum Kind { SYNC, FRAME, RESET } kind;
    dabgpu_rx_member* m;
    int stage;
    size_t sample;
    float beta;
    uint64_t gen;
    int want_views, tie;
    dabgpu_sync_cfg cfg;
    const float* d_iq;              // FRAME: the member's upload buffer that holds the samples
    int up;                         // FRAME: the upload stream the member's copy went to
};

struct dabgpu_rx_member {
    dabgpu_rx_bank* bank = nullptr;
    int slot = -1;
    dabgpu_frame_session* ses = nullptr;        // the member's result store (what the decoders fetch from); the device half makes and fills it
    float* const* h_stage = nullptr;            // the receiver's staging buffers
    rx_member_device* dev = nullptr;
    // reader -> worker -> completer, all under the bank's mutex
    int sync_state = 0;                         // 0 none, 1 posted, 2 enqueued, 3 done
    int sync_status = DABGPU_OK;
    bool sync_coarse = false;
    dabgpu_sync_state sync_rec;
    std::vector<float> sync_imp, sync_frq;
    int stage_state[3] = {0, 0, 0};             // 0 free, 2 a frame was posted from it: its upload is enqueued
    uint64_t next_gen = 0;                      // next generation to post
    uint64_t done_gen = 0;                      // generations < done_gen have their results in the session's slots
    int frame_status[RX_BANK_SLOTS] = {0};      // of generation gen at gen % RX_BANK_SLOTS, written when its round is handed out: a failed round fails its own frames only
    int jobs_in_flight = 0;
    std::condition_variable cv;                 // the member's own threads wait here (on the bank's mutex): a hand-out wakes the members it concerns, not all of them
    double last_post_us = -1e18;                // when the member posted last (the worker's gathering rule)
    double last_record_us = -1e18;              // when a synchroniser's record was handed to the member last, and whether it has posted a frame since
    bool posted_since_record = true;
};

// the scheduling half of a round (the device keeps its buffers and events of round `no` at no % RX_BANK_TICKS)
struct rx_bank_round {
    uint64_t no = 0;
    std::vector<rx_bank_job> sync_jobs, frame_jobs, resets;
    std::vector<dabgpu_subchannel> subs; std::vector<uint32_t> sub_off, sub_n; uint32_t cif_out = 0; bool fic = false;   // the subscription when the round was formed
    int status = -1;                            // -1: not enqueued yet
    bool busy = false;                          // enqueued, not yet handed out by the completers
    bool sync_handed = false;                   // the synchronisers' records of the round are with their members
};

// What the scheduler asks of the device.  The worker thread calls enqueue; the two completer threads the waits and hand-overs of their kind, round by
// round in order; the members' own threads upload / wait_stage / fetch_frame / member_*.  `st` is the round's status so far; a hand-over returns it, or
// its own failure.
struct rx_bank_device {
    virtual ~rx_bank_device() {}                                              // waits for the device, frees the bank's buffers
    virtual void bind_thread() = 0;                                           // a scheduler thread starts
    virtual int member_open(dabgpu_rx_member* m) = 0;                         // m has its slot; makes m->ses, m->dev (released again on failure)
    virtual void member_close(dabgpu_rx_member* m) = 0;
    virtual float* prs_row(int slot) = 0;                                     // DABGPU_NB_FFT complex samples: the member copies its PRS here when it posts a synchroniser
    virtual int enqueue(const rx_bank_round& t) = 0;                          // the resets, then the round
    virtual int wait_sync(const rx_bank_round& t) = 0;
    virtual void hand_sync(const rx_bank_round& t, size_t k) = 0;             // record of t.sync_jobs[k] -> its member's sync_rec / sync_imp / sync_frq (bank mutex held)
    virtual int wait_frames(const rx_bank_round& t) = 0;
    virtual int deliver_frame(const rx_bank_round& t, size_t j, int st) = 0;  // results of t.frame_jobs[j] -> its member's result slot
    virtual int upload(dabgpu_rx_member* m, int stage, size_t frame_sample, uint64_t gen, int up, const float** d_iq) = 0;
    virtual int wait_stage(dabgpu_rx_member* m, int stage) = 0;               // the upload from that staging buffer has finished
    virtual void drain_uploads() = 0;
    virtual int fetch_frame(dabgpu_rx_member* m, uint64_t gen, dabgpu_receiver_frame* out) = 0;   // a delivered generation's result slot
};
// the device half of a new bank (receiver_bank.hip; the CPU tests link their own)
int dabgpu_rx_bank_device_open(int device, rx_bank_device** out);
// tests: members in the slot table and the reference count of a device's bank (-1, -1: no bank)
void dabgpu_rx_bank_census(int device, int* members, int* refs);

// The launches of a batched entry: how a call on nbatch columns becomes launches of the level's widths, shared by the
// sampler and the Darcy handle.  The entry lists its per-column operands once; for every launch of nb columns starting at
// column `done` the body finds the pointer to use in Chunk::dev, in the order listed:
//   In / Out   sample-major device arrays of the kernels.  Device memspace: the caller's array at column `done`.  Host
//              memspace: `stage`, uploaded before the body (In) or copied back behind it (Out).
//   Made       an output the body leaves in a device buffer of the handle: the body sets dev[i], and it is copied out
//              behind the body in both memspaces (device to device or device to host).  MadeHost: the caller's array is
//              host memory whatever the memspace.
//   Host       a host array with one entry of `len` per column (stats, Q, status words): the offset only.
// An absent optional operand (user == NULL) yields NULL and is never copied.  Uploads and copies run in the listed order.
// Operands may share a staging buffer (an input the body has consumed before it writes the output staged there, or an
// array that is read and written in place listed as an In and an Out): every staging buffer of a launch is sized before
// the first upload of that launch, so no upload is lost to a later operand's DevBuf::ensure.
#pragma once
#include "common.hpp"

#include <functional>

namespace pmc {

struct ChunkArg {
    enum Kind { In, Out, Made, MadeHost, Host } kind;
    const void* user;                 // the caller's array, all columns
    size_t len, size;                 // entries per column, bytes per entry
    DevBuf<double>* stage = nullptr;  // In / Out
    static ChunkArg in(const double* p, size_t len, DevBuf<double>& stage) { return {In, p, len, sizeof(double), &stage}; }
    static ChunkArg out(double* p, size_t len, DevBuf<double>& stage) { return {Out, p, len, sizeof(double), &stage}; }
    template <class T>
    static ChunkArg made(T* p, size_t len) { return {Made, p, len, sizeof(T)}; }
    template <class T>
    static ChunkArg made_host(T* p, size_t len) { return {MadeHost, p, len, sizeof(T)}; }
    template <class T>
    static ChunkArg host(T* p, size_t len) { return {Host, p, len, sizeof(T)}; }
    static ChunkArg stats(pmc_stats* p) { return host(p, 1); }
};
struct Chunk {
    int done, nb;
    void** dev;
    template <class T>
    T* at(int i) const { return static_cast<T*>(dev[i]); }
};

// width of the first launch of a call on nbatch columns at a level whose launches carry `width` (batch_width): the widest
// width, halved until it fits.  Every later launch of the call is narrower or equal, and DevBuf::ensure never shrinks: what
// an entry sizes for this width ahead of the driver serves the whole call.
inline int first_chunk(int width, int nbatch) {
    int nb = width;
    while (nb > nbatch) nb >>= 1;
    return nb;
}

// The launches, each the widest that fits what is left.  sync_every_launch: the stream is synchronised behind every launch
// (and its copies); false: nowhere here.  The entry says which, the driver does not decide it.
inline void for_chunks(Ctx& ctx, int width, int nbatch, int memspace, bool sync_every_launch, const std::vector<ChunkArg>& args,
                       const std::function<void(const Chunk&)>& body) {
    hipStream_t st = ctx.stream;
    const bool host = memspace == PMC_MEM_HOST;
    std::vector<void*> dev(args.size());
    int done = 0;
    while (done < nbatch) {
        const int nb = first_chunk(width, nbatch - done);
        auto user = [&](const ChunkArg& a) { return a.user ? (char*)a.user + (size_t)done * a.len * a.size : nullptr; };
        auto staged = [&](const ChunkArg& a) { return host && a.user && (a.kind == ChunkArg::In || a.kind == ChunkArg::Out); };
        for (const ChunkArg& a : args)
            if (staged(a)) a.stage->ensure(a.len * nb);
        for (size_t i = 0; i < args.size(); ++i) {
            const ChunkArg& a = args[i];
            const bool made = a.kind == ChunkArg::Made || a.kind == ChunkArg::MadeHost;
            dev[i] = made ? nullptr : user(a);
            if (!staged(a)) continue;
            if (a.kind == ChunkArg::In) PMC_HIP(hipMemcpyAsync(a.stage->p, dev[i], a.size * a.len * nb, hipMemcpyHostToDevice, st));
            dev[i] = a.stage->p;
        }
        body(Chunk{done, nb, dev.data()});
        for (size_t i = 0; i < args.size(); ++i) {
            const ChunkArg& a = args[i];
            const bool made = a.kind == ChunkArg::Made || a.kind == ChunkArg::MadeHost;
            if (!user(a) || !(made || (host && a.kind == ChunkArg::Out))) continue;
            const bool to_host = host || a.kind == ChunkArg::MadeHost;
            PMC_REQUIRE(dev[i] != nullptr, "for_chunks: the body left an output it makes unset");
            PMC_HIP(hipMemcpyAsync(user(a), dev[i], a.size * a.len * nb, to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
        }
        if (sync_every_launch) PMC_HIP(hipStreamSynchronize(st));
        done += nb;
    }
}

}  // namespace pmc

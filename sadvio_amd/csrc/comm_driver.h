// comm_driver.h — the built-in collective of a window sharded over several GPUs: RCCL, loaded on first use (single-GPU solves never
// touch it), its all-reduce as the handle's hook, and the bodies of comm_init_rccl, comm_info and rccl_unique_id.
// Part of the library's single translation unit (ba_capi.hip); not a public header.
#pragma once
#include "ba_handle.h"

namespace {

std::string load_rccl(RcclLib& R) {
    if (R.lib) return "";
    R.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!R.lib) R.lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!R.lib) return std::string("dlopen librccl: ") + dlerror();
    R.get_id = (int (*)(NcclId*))dlsym(R.lib, "ncclGetUniqueId");
    R.init_rank = (int (*)(void**, int, NcclId, int))dlsym(R.lib, "ncclCommInitRank");
    R.all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(R.lib, "ncclAllReduce");
    R.destroy = (int (*)(void*))dlsym(R.lib, "ncclCommDestroy");
    R.err_string = (const char* (*)(int))dlsym(R.lib, "ncclGetErrorString");
    R.comm_count = (int (*)(void*, int*))dlsym(R.lib, "ncclCommCount");
    R.comm_user_rank = (int (*)(void*, int*))dlsym(R.lib, "ncclCommUserRank");
    R.comm_cu_device = (int (*)(void*, int*))dlsym(R.lib, "ncclCommCuDevice");
    if (!R.get_id || !R.init_rank || !R.all_reduce || !R.destroy) return "missing RCCL symbol";
    return "";
}
int rccl_allreduce(void* ctx, double* buf, int64_t count, void* stream) {
    sadvio_ba_handle* h = (sadvio_ba_handle*)ctx;
    // ncclDouble = 8, ncclSum = 0; in place
    return h->rccl.all_reduce(buf, buf, (size_t)count, 8, 0, h->rccl.comm, (hipStream_t)stream);
}

int rccl_unique_id(void* id128) {
    RcclLib R;
    const std::string e = load_rccl(R);
    if (!e.empty()) return SADVIO_E_RCCL;
    NcclId id;
    if (R.get_id(&id) != 0) return SADVIO_E_RCCL;
    memcpy(id128, &id, sizeof(id));
    return SADVIO_OK;  // the library stays loaded (process lifetime)
}

int comm_init_rccl(sadvio_ba_handle* h, int32_t rank, int32_t world, const void* id128) {
    HIP_TRY(hipSetDevice(h->device));
    const std::string e = load_rccl(h->rccl);
    if (!e.empty()) { h->err = "comm_init_rccl: " + e; return SADVIO_E_RCCL; }
    NcclId id;
    memcpy(&id, id128, sizeof(id));
    const int rc = h->rccl.init_rank(&h->rccl.comm, world, id, rank);
    if (rc != 0) {
        h->err = std::string("comm_init_rccl: ncclCommInitRank: ") + (h->rccl.err_string ? h->rccl.err_string(rc) : "error");
        h->rccl.comm = nullptr;
        return SADVIO_E_RCCL;
    }
    h->rank = rank; h->world = world; h->coll_fn = rccl_allreduce; h->coll_ctx = h;
    return SADVIO_OK;
}

int comm_info(sadvio_ba_handle* h, int32_t* nranks, int32_t* rank, int32_t* device, int32_t* is_rccl) {
    int n = h->world, r = h->rank, d = h->device;
    const bool rccl = h->rccl.comm != nullptr;
    if (rccl) {   // what the COMMUNICATOR says, not what it was asked for
        if (!h->rccl.comm_count || !h->rccl.comm_user_rank || h->rccl.comm_count(h->rccl.comm, &n) != 0 || h->rccl.comm_user_rank(h->rccl.comm, &r) != 0) {
            h->err = "comm_info: ncclCommCount / ncclCommUserRank failed"; return SADVIO_E_RCCL;
        }
        if (h->rccl.comm_cu_device) (void)h->rccl.comm_cu_device(h->rccl.comm, &d);
    }
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    if (device) *device = d;
    if (is_rccl) *is_rccl = rccl ? 1 : 0;
    return SADVIO_OK;
}

}  // namespace

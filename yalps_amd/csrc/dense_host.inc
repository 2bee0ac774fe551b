// dense_host.inc -- what the hosts of the two dense tensor libraries share: the checks of a call's operands, bounds and pointers,
// the operand's device form, and the adoption of a sibling library's kernels.  Included inside the anonymous namespace of
// lp_dense.hip (libyalps_lpdense.so) and milp_dense.hip (libyalps_milpdense.so) after wg_queue_host.inc.  A library names
// itself with a struct X:
//   X::name     "yalps_lpdense", in messages
//   X::Operand  its C ABI's operand descriptor (ptr, batch, row, col)

// an operand of `rows` x `cols` elements per problem (a vector: cols = 1, the col stride ignored)
template <class X>
int check_operand(const char *name, const typename X::Operand *o, int32_t count, int64_t rows, int64_t cols) {
    const std::string who = std::string(X::name) + ": " + name;
    if (!o) return fail(YALPS_E_ARG, who + ": the operand descriptor is NULL");
    if (o->batch < 0 || o->row < 0 || o->col < 0) return fail(YALPS_E_ARG, who + ": negative stride");
    if (count > 0 && rows > 0 && cols > 0 && !o->ptr) return fail(YALPS_E_ARG, who + " is NULL");
    return 0;
}

template <class X>
int check_operands(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const typename X::Operand *c, const typename X::Operand *A_ub,
                   const typename X::Operand *b_ub, const typename X::Operand *A_eq, const typename X::Operand *b_eq) {
    if (int rc = check_operand<X>("c", c, count, n, 1)) return rc;
    if (int rc = check_operand<X>("A_ub", A_ub, count, m_ub, n)) return rc;
    if (int rc = check_operand<X>("b_ub", b_ub, count, m_ub, 1)) return rc;
    if (int rc = check_operand<X>("A_eq", A_eq, count, m_eq, n)) return rc;
    return check_operand<X>("b_eq", b_eq, count, m_eq, 1);
}

// a HOST list of `len` 0-based variable indices: inside 0 .. n-1 and ascending; entry(t): a further refusal of entry t, or 0
template <class X, class Entry>
int check_index_list(const char *name, int32_t len, const int32_t *idx, int32_t n, Entry entry) {
    const std::string who = std::string(X::name) + ": " + name;
    if (len > 0 && !idx) return fail(YALPS_E_ARG, who + " is NULL");
    for (int32_t t = 0; t < len; t++) {
        if (idx[t] < 0 || idx[t] >= n)
            return fail(YALPS_E_ARG, who + "[" + std::to_string(t) + "] = " + std::to_string(idx[t]) + " is outside 0 .. n-1");
        if (t && idx[t] <= idx[t - 1]) return fail(YALPS_E_ARG, who + " is not ascending at " + std::to_string(t));
        if (int rc = entry(t)) return rc;
    }
    return 0;
}

// the bounds of a call: lb / ub may be NULL descriptors (absent); upper_idx is host memory
template <class X, class Entry>
int check_bounds(int32_t count, int32_t n, const typename X::Operand *lb, const typename X::Operand *ub, int32_t n_upper, const int32_t *upper_idx,
                 Entry entry) {
    if (lb)
        if (int rc = check_operand<X>("lb", lb, count, n, 1)) return rc;
    if (ub)
        if (int rc = check_operand<X>("ub", ub, count, n_upper, 1)) return rc;
    if (n_upper > 0 && !ub) return fail(YALPS_E_ARG, std::string(X::name) + ": n_upper > 0 without ub");
    return check_index_list<X>("upper_idx", n_upper, upper_idx, n, entry);
}

// A pointer a kernel is to dereference: device (or managed) memory of the handle's device, known to THIS runtime.
int check_pointer(int device, const char *entry, const char *name, const void *p) {
    if (!p) return 0;
    const std::string who = std::string(entry) + ": " + name;
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof attr);
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError(); // (the lookup's failure is this answer, not the next call's)
        return fail(YALPS_E_ARG, who + " is a pointer this HIP runtime does not know (host memory, or memory of another HIP runtime "
                                       "in this process: load the framework that owns it before this library)");
    }
    if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)
        return fail(YALPS_E_ARG, who + " is host memory: operands and outputs are device pointers");
    if (attr.type == hipMemoryTypeDevice && attr.device != device)
        return fail(YALPS_E_ARG, who + " is memory of device " + std::to_string(attr.device) + ", the handle is on device " + std::to_string(device));
    return 0;
}

template <class Operand>
DenseOperand operand(const Operand *o, bool vector) {
    return DenseOperand{o->ptr, (long long)o->batch, (long long)o->row, vector ? 0ll : (long long)o->col};
}

// `own`, the library's table of its plain kernels, over the six forms a sibling library hands out (its *_forms, in
// QUEUE_KERNEL_TABLE's order): the sibling's code object holds them, this library launches them.  *seventh: the kernel a
// MILP sibling hands out behind them, its epilogue.
template <class LaunchT>
KernelTable<LaunchT> adopt_forms(const KernelTable<LaunchT> &own, const char *name, void (*forms)(void **), void **seventh = nullptr) {
    KernelTable<LaunchT> t = own;
    t.name = name;
    void *fn[7] = {};
    forms(fn);
    for (int k = 0; k < 6; k++) t.forms[k].fn = reinterpret_cast<void (*)(LaunchT)>(fn[k]);
    if (seventh) *seventh = fn[6];
    return t;
}

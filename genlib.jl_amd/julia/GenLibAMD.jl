# GenLibAMD.jl -- drop-in MI355X path for GenLib.jl's dense kinship matrix.
#
# `GenLibAMD.phi` has the signature, keyword arguments, printed lines, return type and error
# behaviour of `GenLib.phi(pedigree::Pedigree, probandIDs; verbose, compute)`
# (GenLib.jl v0.1.4, src/compute.jl:233-304); the level sweep (src/compute.jl:269-303) runs
# in libgenphi.so (include/genphi.h) on the GPU instead of under Threads.@threads.
# Everything else (gen.genealogy, gen.pro, the Pedigree container) stays GenLib.jl's own.
#
# NOT exercised in the build container (no Julia there, nor on the GPU boxes); see INTEGRATION.md.
module GenLibAMD

import GenLib
import Random, Statistics                  # (standard library: phiCI / fCI draw a seed and take quantiles)

const libgenphi = get(ENV, "GENPHI_LIB", joinpath(@__DIR__, "..", "lib", "libgenphi.so"))

struct GenphiOpts              # mirrors genphi_opts (include/genphi.h)
    device::Int32
    kernel::Int32
    row_begin::Int64
    row_end::Int64
    timing::Int32
    flags::Int32               # GENPHI_FLAG_*: 1 = no hipGraph replay, 2 = Float64 level matrices (GENPHI_FLAG_STORAGE_F64)
end
const FLAG_STORAGE_F64 = Int32(2)

last_error() = unsafe_string(ccall((:genphi_last_error, libgenphi), Cstring, ()))

function check(rc::Cint)
    rc == 0 && return
    msg = last_error()
    # GENPHI_ERR_UNKNOWN_ID / GENPHI_ERR_ORDER are KeyErrors in the reference
    (rc == 1 || rc == 2) ? throw(KeyError(msg)) : error("libgenphi: $msg (code $rc)")
end

# flatten in rank order (the traversal of GenLib.genout, src/output.jl:24-29, kept at 64 bit)
function flatten(pedigree::GenLib.Pedigree)
    n = length(pedigree)
    ind = Vector{Int64}(undef, n); father = zeros(Int64, n); mother = zeros(Int64, n)
    sex = Vector{Int64}(undef, n)
    for (k, individual) in enumerate(values(pedigree))
        ind[k] = individual.ID
        sex[k] = individual.sex
        isnothing(individual.father) || (father[k] = individual.father.ID)
        isnothing(individual.mother) || (mother[k] = individual.mother.ID)
    end
    ind, father, mother, sex
end

# The plans of the last calls, per pedigree: the host prologue of GenLib.phi (src/compute.jl:236-262: levelisation, cut sets, index copy)
# depends on (pedigree, probandIDs) alone, so a repeated call skips planning, upload and the calibration of the sparse cuts and pays the
# sweep and the copy (genea140: 6.2 ms for a first call, 0.7 ms for a repeated one).  A plan that holds more than PLAN_CACHE_DEVICE_BYTES
# of device memory is destroyed at the end of its call.  `release_cached()` drops the plans and what the library itself keeps.
const PLAN_CACHE_ENTRIES = 4
const PLAN_CACHE_DEVICE_BYTES = 2 << 30
const plan_cache = WeakKeyDict{GenLib.Pedigree, Vector{Tuple{Vector{Int}, Int, Ptr{Cvoid}}}}()   # (probandIDs, device, plan), least recent first

destroy_plan(plan::Ptr{Cvoid}) = ccall((:genphi_plan_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), plan)

function release_cached()
    for entries in values(plan_cache), (_, _, plan) in entries
        destroy_plan(plan)
    end
    empty!(plan_cache)
    ccall((:genphi_release_cached, libgenphi), Cvoid, ())      # device blocks, streams and pinned staging the library keeps between calls
end

# tuning: nothing (the library's defaults; GENPHI_* environment hooks only under GENPHI_ENV_HOOKS=1) or settings for this plan alone,
# e.g. Dict("SPARSE_K" => -1) (genphi_plan_create_tuned; such plans are not cached)
function create_plan(pedigree::GenLib.Pedigree, probandIDs::Vector{Int}, tuning)
    ind, father, mother, _ = flatten(pedigree)
    plan = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother probandIDs begin
        if isnothing(tuning)
            check(ccall((:genphi_plan_create, libgenphi), Cint,
                        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Ptr{Cvoid}}),
                        length(ind), ind, father, mother, length(probandIDs), probandIDs, plan))
        else
            t = ccall((:genphi_tuning_create, libgenphi), Ptr{Cvoid}, ())
            try
                for (name, value) in tuning
                    check(ccall((:genphi_tuning_set, libgenphi), Cint, (Ptr{Cvoid}, Cstring, Cstring), t, string(name), string(value)))
                end
                check(ccall((:genphi_plan_create_tuned, libgenphi), Cint,
                            (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}),
                            length(ind), ind, father, mother, length(probandIDs), probandIDs, t, plan))
            finally
                ccall((:genphi_tuning_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), t)
            end
        end
    end
    plan[]
end

"""
    phi(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree);
        verbose::Bool = false, compute::Bool = true, device::Integer = -1, tuning = nothing)

Square `Matrix{Float32}` of pairwise kinship coefficients between probands, bit-identical to
`GenLib.phi`, computed on an MI355X.
"""
function phi(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree);
             verbose::Bool = false, compute::Bool = true, device::Integer = -1, tuning = nothing)
    entries = get!(() -> Tuple{Vector{Int}, Int, Ptr{Cvoid}}[], plan_cache, pedigree)
    hit = isnothing(tuning) ? findfirst(e -> e[2] == device && e[1] == probandIDs, entries) : nothing
    plan = Ref{Ptr{Cvoid}}(isnothing(hit) ? create_plan(pedigree, probandIDs, tuning) : entries[hit][3])
    isnothing(hit) || deleteat!(entries, hit)              # (re-inserted as the most recent one below, if the call succeeds)
    keep = false
    try
        nlev = Ref{Int32}(0); sizes = Ref{Ptr{Int64}}(C_NULL); both = Ref{Ptr{Int64}}(C_NULL)
        check(ccall((:genphi_plan_levels, libgenphi), Cint,
                    (Ptr{Cvoid}, Ptr{Int32}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}), plan[], nlev, sizes, both))
        nsteps = max(nlev[] - 1, 0)
        cut = unsafe_wrap(Array, sizes[], Int(nlev[])); dragged = unsafe_wrap(Array, both[], nsteps)
        if verbose || !compute                           # lines of src/compute.jl:257-260
            for i in 1:nsteps
                println("Step $i of $nsteps: $(cut[i]) founders, $(cut[i+1]) probands, $(dragged[i]) both.")
            end
        end
        compute || return nothing                        # src/compute.jl:264-266
        hook = nothing
        if verbose                                       # lines of src/compute.jl:281-284, printed INSIDE the level loop as there:
            # the library calls back right before it hands each level step to the GPU (genphi_plan_set_step_hook)
            hook = @cfunction($((step, n, _) -> (println("Running step $(step + 1) of $n ($(cut[step+1]) founders, $(cut[step+2]) probands, $(dragged[step+1]) both."); nothing)),
                              Cvoid, (Int32, Int32, Ptr{Cvoid}))
            check(ccall((:genphi_plan_set_step_hook, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), plan[], hook, C_NULL))
        end
        N = Int(ccall((:genphi_plan_n_probands, libgenphi), Int64, (Ptr{Cvoid},), plan[]))
        Φ = Matrix{Float32}(undef, N, N)                 # symmetric: row-major == column-major
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        GC.@preserve Φ hook check(ccall((:genphi_compute_f32, libgenphi), Cint,
                                   (Ptr{Cvoid}, Ptr{Float32}, Ptr{GenphiOpts}, Ptr{Cvoid}),
                                   plan[], Φ, opts, C_NULL))
        isnothing(hook) || check(ccall((:genphi_plan_set_step_hook, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), plan[], C_NULL, C_NULL))
        if isnothing(tuning) && ccall((:genphi_plan_device_bytes, libgenphi), Int64, (Ptr{Cvoid},), plan[]) <= PLAN_CACHE_DEVICE_BYTES
            push!(entries, (copy(probandIDs), Int(device), plan[]))
            keep = true
            while length(entries) > PLAN_CACHE_ENTRIES
                destroy_plan(popfirst!(entries)[3])
            end
        end
        return Φ
    finally
        keep || destroy_plan(plan[])
    end
end

"""
    phi(individualᵢ::GenLib.Individual, individualⱼ::GenLib.Individual, pedigree::GenLib.Pedigree; device = -1)

Float64 kinship of a pair, as `GenLib.phi(individualᵢ, individualⱼ)` (src/compute.jl:66-95), from one
Float64 level sweep on the GPU instead of the un-memoised recursion.  (The reference's method needs no
pedigree argument because its `Individual`s carry pointers to their parents; the flat arrays the
library takes are built from the pedigree.)  Bit-identical while kinships are exactly representable in
Float64 (pedigrees less than ~26 generations deep); beyond, within 2 L 2^-53 relative of the exact
kinship after L level steps (subnormal results within 4 x 2^-1074).
"""
function phi(individualᵢ::GenLib.Individual, individualⱼ::GenLib.Individual, pedigree::GenLib.Pedigree;
             device::Integer = -1)
    ind, father, mother, _ = flatten(pedigree)
    a = Int64[individualᵢ.ID]; b = Int64[individualⱼ.ID]; out = Vector{Float64}(undef, 1)
    GC.@preserve ind father mother a b out check(ccall((:genphi_phi_pairs, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int32),
        length(ind), ind, father, mother, 1, a, b, out, Int32(device)))
    out[1]
end

"""
    f(pedigree::GenLib.Pedigree, IDs::Vector{Int}; device::Integer = -1)

Coefficients of inbreeding (`Vector{Float32}`), as `GenLib.f` (src/compute.jl:500-511), from ONE
Float64 level sweep over the parents on the GPU plus point lookups, instead of one un-memoised
pairwise recursion per individual; rounded to Float32 once, like the reference.
"""
function f(pedigree::GenLib.Pedigree, IDs::Vector{Int}; device::Integer = -1)
    coefficients = zeros(Float32, length(IDs))
    pairs = [(pedigree[ID].father, pedigree[ID].mother) for ID in IDs]       # KeyError on unknown ID
    known = findall(p -> !isnothing(p[1]) && !isnothing(p[2]), pairs)
    isempty(known) && return coefficients
    parents = sort(unique(vcat([pairs[k][1].ID for k in known], [pairs[k][2].ID for k in known])))
    rows = Int64[searchsortedfirst(parents, pairs[k][1].ID) - 1 for k in known]
    cols = Int64[searchsortedfirst(parents, pairs[k][2].ID) - 1 for k in known]
    ind, father, mother, _ = flatten(pedigree)
    plan = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother parents begin
        check(ccall((:genphi_plan_create, libgenphi), Cint,
                    (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Ptr{Cvoid}}),
                    length(ind), ind, father, mother, length(parents), parents, plan))
    end
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, FLAG_STORAGE_F64))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}),
                    plan[], opts, C_NULL))
        values64 = Vector{Float64}(undef, length(known))
        GC.@preserve rows cols values64 check(ccall((:genphi_result_entries, libgenphi), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}), plan[], length(known), rows, cols, values64))
        coefficients[known] .= Float32.(values64)
    finally
        ccall((:genphi_plan_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), plan[])
    end
    coefficients
end

"""
    phiMeanGroups(pedigree::GenLib.Pedigree, groups::Dict{Int, String}, probandIDs::Vector{Int} = collect(keys(groups));
                  device::Integer = -1)

Mean kinship within and between groups of probands (e.g. `GenLib._pop(GenLib.pop140)`): `(names, sizes, mean)` with the
names sorted and `mean` a `Matrix{Float64}`; `mean[a, a]` is `phiMean` (src/compute.jl:454-459) of the block of group `a`,
`mean[a, b]` the plain mean of the block between `a` and `b`, `NaN` where there is no pair.  The matrix stays on the GPU:
`genphi_result_group_sums` reduces it there.  Probands that are not in `groups` take part in the sweep but belong to no group.
"""
function phiMeanGroups(pedigree::GenLib.Pedigree, groups::Dict{Int, String}, probandIDs::Vector{Int} = collect(keys(groups));
                       device::Integer = -1)
    isempty(groups) && throw(ArgumentError("groups is empty"))
    names = sort(unique(values(groups)))
    index = Dict(name => Int32(k - 1) for (k, name) in enumerate(names))
    label(ID) = haskey(groups, ID) ? index[groups[ID]] : Int32(-1)
    # by (group name, ID), probands in no group last: every group is one run (form 0 of genphi_result_group_sums)
    ordered = sort(unique(probandIDs), by = ID -> (label(ID) < 0 ? length(names) : Int(label(ID)), ID))
    labels = Int32[label(ID) for ID in ordered]
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    G = length(names)
    plan = create_plan(pedigree, ordered, nothing)
    sums = Matrix{Float64}(undef, G, G); diagonal = Vector{Float64}(undef, G); sizes = Vector{Int64}(undef, G)
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}), plan, opts, C_NULL))
        GC.@preserve labels sums diagonal sizes check(ccall((:genphi_result_group_sums, libgenphi), Cint,
            (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}),
            plan, Int32(G), labels, sums, diagonal, C_NULL, sizes, C_NULL))
    finally
        destroy_plan(plan)
    end
    # (sums arrives row-major: the transpose of the Julia matrix; all rows are resident, so it is symmetric up to the order of additions)
    mean = Matrix{Float64}(undef, G, G)
    for a in 1:G, b in 1:G
        pairs = a == b ? sizes[a] * (sizes[a] - 1) : sizes[a] * sizes[b]
        total = a == b ? sums[a, a] - diagonal[a] : sums[a, b]
        mean[b, a] = pairs > 0 ? total / pairs : NaN
    end
    (names = names, sizes = sizes, mean = mean)
end

"""
    phiOver(pedigree::GenLib.Pedigree, threshold::Real, probandIDs::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1)

GENLIB's `gen.phiOver`: the pairs of probands with kinship at or above `threshold`, as `(row, col, pro1, pro2, kinship)`: positions
`row < col` in the order of `unique(probandIDs)` (1-based here), the IDs at those positions and the `Float32` entries of `phi`, sorted
by row, then column; each pair once.  The matrix stays on the GPU: `genphi_result_over` selects there, in two passes over its upper
triangle (count, then write).  The reference has no `phiOver`; the definition (`>=`, the strict upper triangle, row-major order) is
this package's own.
"""
function phiOver(pedigree::GenLib.Pedigree, threshold::Real, probandIDs::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1)
    isnan(threshold) && throw(ArgumentError("the threshold is NaN"))
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    plan = create_plan(pedigree, ordered, nothing)
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}), plan, opts, C_NULL))
        n = Ref{Int64}(0)
        over(cap, rows, cols, values) = check(ccall((:genphi_result_over, libgenphi), Cint,
            (Ptr{Cvoid}, Float64, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Int64}),
            plan, Float64(threshold), cap, rows, cols, values, n))
        over(0, C_NULL, C_NULL, C_NULL)                                     # count only
        rows = Vector{Int32}(undef, n[]); cols = Vector{Int32}(undef, n[]); kinship = Vector{Float32}(undef, n[])
        GC.@preserve rows cols kinship over(length(rows), rows, cols, kinship)
        row = Int.(rows) .+ 1; col = Int.(cols) .+ 1
        return (row = row, col = col, pro1 = ordered[row], pro2 = ordered[col], kinship = kinship)
    finally
        destroy_plan(plan)
    end
end

"""
    phiClusters(pedigree::GenLib.Pedigree, threshold::Real, probandIDs::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1)

The families at a kinship cutoff: the connected components of the graph whose edges are the pairs of probands with kinship at or above
`threshold` (`phiOver`'s rule), as `(pro, label, cluster, sizes, n_pairs)`: `label[i]` is the smallest position (1-based here, in the
order of `unique(probandIDs)`) in `i`'s component, `cluster[i]` its dense number `1 .. K` in the order of each cluster's first member,
`sizes` the `K` cluster sizes and `n_pairs` the number of edges.  The matrix stays on the GPU and the pairs are never listed:
`genphi_result_clusters` runs a lock-free union-find there over one read of its upper triangle.  The reference has no such function;
the definition is this package's own (`include/genphi.h`).
"""
function phiClusters(pedigree::GenLib.Pedigree, threshold::Real, probandIDs::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1)
    isnan(threshold) && throw(ArgumentError("the threshold is NaN"))
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    plan = create_plan(pedigree, ordered, nothing)
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}), plan, opts, C_NULL))
        labels = Vector{Int32}(undef, length(ordered)); k = Ref{Int64}(0); n = Ref{Int64}(0)
        GC.@preserve labels check(ccall((:genphi_result_clusters, libgenphi), Cint, (Ptr{Cvoid}, Float64, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}),
            plan, Float64(threshold), labels, k, n))
        label = Int.(labels) .+ 1
        firsts = findall(i -> label[i] == i, eachindex(label))              # ascending: the order of each cluster's first member
        number = zeros(Int, length(label)); number[firsts] = 1:length(firsts)
        cluster = number[label]
        sizes = zeros(Int64, length(firsts)); foreach(c -> sizes[c] += 1, cluster)
        return (pro = ordered, label = label, cluster = cluster, sizes = sizes, n_pairs = n[])
    finally
        destroy_plan(plan)
    end
end

"""
    phiTree(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree); floor::Real = nextfloat(0.0f0),
            device::Integer = -1)

The single-linkage tree of the kinships -- the families of `phiClusters` at every cutoff at once -- as
`(pro, row, col, pro1, pro2, kinship, floor, n_trees, rounds)`: the edges of the maximum spanning forest of the graph whose edges are the
pairs of probands with kinship at or above `floor` (`phiOver`'s rule; the default is the smallest positive `Float32`, "any positive
kinship"), ordered by larger kinship first, then smaller `row`, then smaller `col` (positions 1-based here, in the order of
`unique(probandIDs)`; `row < col`).  An edge belongs to the forest iff no path of preceding edges joins its ends, so the answer is unique;
the connected components of the listed edges with kinship `>= t` are `phiClusters`' at `t` for every `t >= floor`.  The matrix stays on
the GPU and the pairs are never listed or sorted: `genphi_result_tree` runs Boruvka's rounds there over the rows of the resident matrix.
The reference has no such function; the definition is this package's own (`include/genphi.h`).  Not run: there is no Julia where this
package is built and tested.
"""
function phiTree(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree); floor::Real = nextfloat(0.0f0),
                 device::Integer = -1)
    isnan(floor) && throw(ArgumentError("the floor is NaN"))
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    plan = create_plan(pedigree, ordered, nothing)
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}), plan, opts, C_NULL))
        slots = max(length(ordered) - 1, 0)
        rows = Vector{Int32}(undef, slots); cols = Vector{Int32}(undef, slots); kinship = Vector{Float32}(undef, slots)
        m = Ref{Int64}(0); trees = Ref{Int64}(0); rounds = Ref{Int32}(0)
        GC.@preserve rows cols kinship check(ccall((:genphi_result_tree, libgenphi), Cint,
            (Ptr{Cvoid}, Float64, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}),
            plan, Float64(floor), rows, cols, kinship, m, trees, rounds))
        row = Int.(rows[1:m[]]) .+ 1; col = Int.(cols[1:m[]]) .+ 1
        return (pro = ordered, row = row, col = col, pro1 = ordered[row], pro2 = ordered[col], kinship = kinship[1:m[]], floor = Float64(floor),
                n_trees = trees[], rounds = Int(rounds[]))
    finally
        destroy_plan(plan)
    end
end

"""
    phiUnrelated(pedigree::GenLib.Pedigree, threshold::Real, probandIDs::Vector{Int} = GenLib.pro(pedigree);
                 priority = :degree, device::Integer = -1)

A maximal set of probands no two of which have kinship at or above `threshold` (the "kinship cutoff" of association studies), as
`(pro, keep, index, kept, degree, rounds)`.  The set is the answer of the sequential greedy rule: visit the probands in ascending order
of `(priority[i], i)` and keep one iff none of its relatives has been kept.  `priority`: `:degree` (the number of relatives at or above
the threshold: the fewest relatives first), `:position` (earlier probands win) or one integer in the `Int32` range per entry of
`unique(probandIDs)`, smaller kept first.  `degree[i]` is that number of relatives, `rounds` the launches the device took.  The matrix
stays on the GPU: `genphi_result_unrelated` finds the set there in rounds over the rows.  The reference has no such function; the
definition is this package's own (`include/genphi.h`).
"""
function phiUnrelated(pedigree::GenLib.Pedigree, threshold::Real, probandIDs::Vector{Int} = GenLib.pro(pedigree);
                      priority = :degree, device::Integer = -1)
    isnan(threshold) && throw(ArgumentError("the threshold is NaN"))
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    if priority isa Symbol
        priority in (:degree, :position) || throw(ArgumentError("priority: :degree, :position or one integer per proband"))
        pri = priority == :degree ? nothing : zeros(Int32, length(ordered))
    else
        length(priority) == length(ordered) || throw(ArgumentError("priority must hold one entry per proband ($(length(ordered)))"))
        pri = Vector{Int32}(priority)                                       # InexactError outside the Int32 range or for a non-integer
    end
    plan = create_plan(pedigree, ordered, nothing)
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}), plan, opts, C_NULL))
        member = Vector{UInt8}(undef, length(ordered)); degree = Vector{Int32}(undef, length(ordered))
        kept = Ref{Int64}(0); rounds = Ref{Int32}(0)
        GC.@preserve pri member degree check(ccall((:genphi_result_unrelated, libgenphi), Cint,
            (Ptr{Cvoid}, Float64, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}),
            plan, Float64(threshold), pri === nothing ? C_NULL : pointer(pri), member, degree, kept, rounds))
        keep = member .== 1
        index = findall(keep)
        return (pro = ordered, keep = keep, index = index, kept = ordered[index], degree = Int.(degree), rounds = Int(rounds[]))
    finally
        destroy_plan(plan)
    end
end

"""
    phiHist(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree); bins = 64, range = (0.0, 0.5), device::Integer = -1)

The distribution of the pairwise kinships: the histogram of `phi[i, j]` over all pairs `i < j` of `unique(probandIDs)`, as
`(edges, counts, below, above, n_pairs)`.  `bins` is a number of uniform bins over `range` or a vector of strictly increasing edges;
a bin holds `edges[b] <= x < edges[b + 1]`, the last one also `x == edges[end]`; `below` and `above` count the pairs outside the edges.
The matrix stays on the GPU: `genphi_result_hist` counts there in one pass over its upper triangle.  The reference has no `phiHist`;
the definition is this package's own (`include/genphi.h`).  The labelled form (counts within and between groups) is reached through
the same entry point with `n_groups` and `group`; this shim does not wrap it.  Uniform edges are computed here as
`first + b * (last - first) / bins` with the last one set to `last`, the arithmetic of `numpy.linspace`, so that both shims hand the same
doubles to the library and agree on an entry that ties with an edge.
"""
function phiHist(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree); bins = 64, range = (0.0, 0.5), device::Integer = -1)
    if bins isa Integer
        bins >= 1 || throw(ArgumentError("bins must be at least 1"))
        lo = Float64(range[1]); hi = Float64(range[2]); step = (hi - lo) / bins
        edges = [lo + b * step for b in 0:bins]
        edges[end] = hi
    else
        edges = Vector{Float64}(bins)
    end
    (2 <= length(edges) <= 4097 && !any(isnan, edges) && all(diff(edges) .> 0)) || throw(ArgumentError("the edges must be 2 .. 4097 strictly increasing numbers"))
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    plan = create_plan(pedigree, ordered, nothing)
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}), plan, opts, C_NULL))
        counts = Vector{Int64}(undef, length(edges) - 1)
        below = Ref{Int64}(0); above = Ref{Int64}(0); n = Ref{Int64}(0)
        GC.@preserve edges counts check(ccall((:genphi_result_hist, libgenphi), Cint,
            (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
            plan, Int32(length(edges)), edges, Int32(0), C_NULL, counts, below, above, n))
        return (edges = edges, counts = counts, below = below[], above = above[], n_pairs = n[])
    finally
        destroy_plan(plan)
    end
end

"""
    phiQuantile(pedigree::GenLib.Pedigree, q, probandIDs::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1)

Quantiles of the pairwise kinships `phi[i, j]`, `i < j`, one `Float64` per entry of `q` (each in `[0, 1]`): with `n` pairs sorted
ascending and `h = q (n - 1)`, `lo + (hi - lo) (h - floor(h))` where `lo` and `hi` are the entries of 0-based rank `floor(h)` and
`ceil(h)` (`Statistics.quantile`'s default).  The matrix stays on the GPU: `genphi_result_select` finds the exact order statistics
there by radix selection, 16 ranks (8 quantiles) per call, four passes over the upper triangle each.
"""
function phiQuantile(pedigree::GenLib.Pedigree, q, probandIDs::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1)
    qs = Float64.(collect(q))
    all(p -> 0 <= p <= 1, qs) || throw(ArgumentError("q must lie in [0, 1]"))
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    plan = create_plan(pedigree, ordered, nothing)
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}), plan, opts, C_NULL))
        n = Ref{Int64}(0)
        check(ccall((:genphi_result_select, libgenphi), Cint, (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float32}, Ptr{Int64}), plan, Int32(0), C_NULL, C_NULL, n))
        n[] >= 1 || throw(ArgumentError("phiQuantile needs at least 2 probands"))
        h = qs .* (n[] - 1)
        out = Vector{Float64}(undef, length(qs))
        for first in 1:8:length(qs)
            part = first:min(first + 7, length(qs))
            ranks = vcat(Int64.(floor.(h[part])), Int64.(ceil.(h[part])))
            values = Vector{Float32}(undef, length(ranks))
            GC.@preserve ranks values check(ccall((:genphi_result_select, libgenphi), Cint, (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float32}, Ptr{Int64}),
                plan, Int32(length(ranks)), ranks, values, C_NULL))
            lo = Float64.(values[1:length(part)]); hi = Float64.(values[length(part)+1:end])
            out[part] = lo .+ (hi .- lo) .* (h[part] .- floor.(h[part]))
        end
        return out
    finally
        destroy_plan(plan)
    end
end

"""
    phiCI(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree); prob = [0.025, 0.05, 0.95, 0.975],
          b::Integer = 5000, seed::Union{Nothing, UInt64} = nothing, device::Integer = -1)

GENLIB's `gen.phiCI`: the bootstrap confidence interval of the mean kinship, as `(prob, quantiles, mean, thetastar, b, seed)`.  A
resample draws the probands with replacement and takes `phiMean` of the resampled matrix; the matrix stays on the GPU:
`genphi_result_bootstrap` draws there (Philox4x32-10 keyed on seed, resample and draw: `include/genphi.h`) and returns, per resample,
the quadratic form of the counts and their weighted diagonal sum, accumulated in `Float64`.  Quantiles are by linear interpolation of
the sorted values (R's type 7).  The reference has no `phiCI`; the definition is this package's own.
"""
function phiCI(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree); prob = [0.025, 0.05, 0.95, 0.975],
               b::Integer = 5000, seed::Union{Nothing, UInt64} = nothing, device::Integer = -1)
    all(p -> 0 <= p <= 1, prob) || throw(ArgumentError("prob must lie in [0, 1]"))
    b >= 1 || throw(ArgumentError("b must be at least 1"))
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    n = length(ordered)
    n >= 2 || throw(ArgumentError("phiCI needs at least 2 probands"))
    s = seed === nothing ? rand(Random.RandomDevice(), UInt64) : seed
    plan = create_plan(pedigree, ordered, nothing)
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}), plan, opts, C_NULL))
        total = Ref{Float64}(0); diagonal = Ref{Float64}(0); rows = Ref{Int64}(0)
        check(ccall((:genphi_result_sums, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}), plan, total, diagonal, rows))
        quad = Vector{Float64}(undef, b); own = Vector{Float64}(undef, b)
        GC.@preserve quad own check(ccall((:genphi_result_bootstrap, libgenphi), Cint,
            (Ptr{Cvoid}, UInt64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}), plan, s, Int32(0), Int32(b), quad, own, C_NULL))
        thetastar = (quad .- own) ./ (Float64(n) * (n - 1))
        return (prob = collect(Float64, prob), quantiles = Statistics.quantile(thetastar, prob), mean = Float32((total[] - diagonal[]) / (n * n - n)),
                thetastar = thetastar, b = Int(b), seed = s)
    finally
        destroy_plan(plan)
    end
end

const MATMUL_MAX_K = 64                    # GENPHI_MATMUL_MAX_K
const EIGEN_MAX_K = 64                     # GENPHI_EIGEN_MAX_K

# the sweep of `ordered`, then query(plan) on its resident result
function with_resident(query, pedigree::GenLib.Pedigree, ordered::Vector{Int}, device::Integer)
    plan = create_plan(pedigree, ordered, nothing)
    try
        opts = Ref(GenphiOpts(Int32(device), 0, 0, 0, 0, 0))
        check(ccall((:genphi_compute_device, libgenphi), Cint, (Ptr{Cvoid}, Ptr{GenphiOpts}, Ptr{Cvoid}), plan, opts, C_NULL))
        return query(plan)
    finally
        destroy_plan(plan)
    end
end

"""
    phiMatmul(pedigree::GenLib.Pedigree, X::AbstractVecOrMat{<:Real}, probandIDs::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1)

The product `Φ * X` of the kinship matrix of the probands with a vector or a tall, skinny matrix `X` (one row per proband, in the order
of `unique(probandIDs)`), as `Float64`.  The matrix stays on the GPU: `genphi_result_matmul` uploads `X` and accumulates in `Float64` by
`fma` in an order that depends on the number of probands alone (`include/genphi.h`), so the same call gives the same bits and a column
does not depend on its neighbours.  More than 64 columns run as blocks of 64.  The reference has no such function.
"""
function phiMatmul(pedigree::GenLib.Pedigree, X::AbstractVecOrMat{<:Real}, probandIDs::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1)
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    n = length(ordered)
    size(X, 1) == n || throw(ArgumentError("X must have one row per proband ($n)"))
    k = size(X, 2)
    xt = Matrix{Float64}(permutedims(reshape(Float64.(X), n, k)))           # k x n column-major = n x k row-major, pitch k
    yt = Matrix{Float64}(undef, k, n)
    with_resident(pedigree, ordered, device) do plan
        for c0 in 1:MATMUL_MAX_K:k
            kk = min(k - c0 + 1, MATMUL_MAX_K)
            GC.@preserve xt yt check(ccall((:genphi_result_matmul, libgenphi), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Int64}),
                plan, Int32(kk), pointer(xt, c0), Int64(k), pointer(yt, c0), Int64(k), C_NULL))
        end
    end
    Y = permutedims(yt)
    return X isa AbstractVector ? vec(Y) : Y
end

"""
    phiSolve(pedigree::GenLib.Pedigree, B::AbstractVecOrMat{<:Real}, probandIDs::Vector{Int} = GenLib.pro(pedigree);
             ridge::Real = 0.0, tol::Real = 1e-10, maxiter::Integer = 1000, device::Integer = -1)

Solves `(Φ + ridge * I) z = B`, the system under the animal model, BLUP and heritability, as
`(solution, residual, iterations, converged, pro)`: conjugate gradients over `genphi_result_matmul` on the resident matrix
(`genphi_result_solve`; the iteration is written out in `include/genphi.h`).  `residual` is the true relative residual
`‖b − (Φ + ridge I) z‖ / ‖b‖` per right-hand side, `iterations` the products it took part in, `converged = residual .<= tol`.
The reference has no such function.
"""
function phiSolve(pedigree::GenLib.Pedigree, B::AbstractVecOrMat{<:Real}, probandIDs::Vector{Int} = GenLib.pro(pedigree);
                  ridge::Real = 0.0, tol::Real = 1e-10, maxiter::Integer = 1000, device::Integer = -1)
    (ridge >= 0 && isfinite(ridge)) || throw(ArgumentError("ridge must be finite and not negative"))
    tol >= 0 || throw(ArgumentError("tol must not be negative or NaN"))
    maxiter >= 1 || throw(ArgumentError("maxiter must be at least 1"))
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    n = length(ordered)
    size(B, 1) == n || throw(ArgumentError("B must have one row per proband ($n)"))
    k = size(B, 2)
    bt = Matrix{Float64}(permutedims(reshape(Float64.(B), n, k)))           # k x n column-major = n x k row-major, pitch k
    zt = zeros(Float64, k, n)
    residual = zeros(Float64, k); iterations = zeros(Int32, k)
    with_resident(pedigree, ordered, device) do plan
        for c0 in 1:MATMUL_MAX_K:k
            kk = min(k - c0 + 1, MATMUL_MAX_K)
            GC.@preserve bt zt residual iterations check(ccall((:genphi_result_solve, libgenphi), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Float64, Float64, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int32}),
                plan, Int32(kk), pointer(bt, c0), Int64(k), Float64(ridge), Float64(tol), Int32(maxiter), pointer(zt, c0), Int64(k),
                pointer(residual, c0), pointer(iterations, c0)))
        end
    end
    Z = permutedims(zt)
    return (solution = B isa AbstractVector ? vec(Z) : Z, residual = residual, iterations = Int.(iterations), converged = residual .<= tol, pro = ordered)
end

"""
    phiEigen(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree);
             k::Integer = 10, center::Bool = false, tol::Real = 1e-8, maxiter::Integer = 300, seed::Integer = 0, device::Integer = -1)

The `k` algebraically largest eigenpairs of the kinship matrix, or with `center = true` of its Gower-centred form `J Φ J`, as
`(values, vectors, residual, converged, products, coordinates, pro)`: Lanczos with full reorthogonalisation whose vectors all stay on
the GPU (`genphi_result_eigen`; the iteration is written out in `include/genphi.h`).  `values` descend, `vectors` is N × k with unit
columns whose component of largest magnitude is positive, `residual` is the true `‖Op v − θ v‖`, `coordinates = vectors .* sqrt.(max.(values, 0))'`
(with `center = true` the principal coordinates).  One Krylov sequence: an eigenvalue repeated among the top k is reported once.
The reference has no such function.  Like the other wrappers of this file, this one has never been run.
"""
function phiEigen(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree);
                  k::Integer = 10, center::Bool = false, tol::Real = 1e-8, maxiter::Integer = 300, seed::Integer = 0, device::Integer = -1)
    tol >= 0 || throw(ArgumentError("tol must not be negative or NaN"))
    ordered = unique(probandIDs)
    foreach(ID -> pedigree[ID], ordered)                                    # KeyError on unknown ID
    n = length(ordered)
    1 <= k <= min(EIGEN_MAX_K, n) || throw(ArgumentError("k must lie in [1, $(min(EIGEN_MAX_K, n))]"))
    k <= maxiter <= 4096 || throw(ArgumentError("maxiter must lie in [k, 4096]"))
    values = zeros(Float64, k); vt = zeros(Float64, k, n)                   # k x n column-major = n x k row-major, pitch k
    residual = zeros(Float64, k); converged = zeros(Int32, k); products = Ref{Int32}(0)
    with_resident(pedigree, ordered, device) do plan
        GC.@preserve values vt residual converged check(ccall((:genphi_result_eigen, libgenphi), Cint,
            (Ptr{Cvoid}, Int32, Int32, Float64, Int32, UInt64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
            plan, Int32(k), Int32(center), Float64(tol), Int32(maxiter), seed % UInt64, pointer(values), pointer(vt), Int64(k),
            pointer(residual), pointer(converged), products))
    end
    V = permutedims(vt)
    return (values = values, vectors = V, residual = residual, converged = converged .!= 0, products = Int(products[]),
            coordinates = V .* sqrt.(max.(values, 0.0))', pro = ordered)
end

"""
    fCI(vectF::AbstractVector{<:Real}; prob = [0.025, 0.05, 0.95, 0.975], b::Integer = 5000, seed::Union{Nothing, UInt64} = nothing)

GENLIB's `gen.fCI`: the bootstrap confidence interval of the mean inbreeding, with `phiCI`'s draws (`genphi_bootstrap_counts`, host only):
the statistic of a resample is the mean of the drawn coefficients.
"""
function fCI(vectF::AbstractVector{<:Real}; prob = [0.025, 0.05, 0.95, 0.975], b::Integer = 5000, seed::Union{Nothing, UInt64} = nothing)
    all(p -> 0 <= p <= 1, prob) || throw(ArgumentError("prob must lie in [0, 1]"))
    b >= 1 || throw(ArgumentError("b must be at least 1"))
    n = length(vectF)
    n >= 2 || throw(ArgumentError("fCI needs at least 2 values"))
    s = seed === nothing ? rand(Random.RandomDevice(), UInt64) : seed
    counts = Matrix{Int32}(undef, n, b)                                     # column r = the counts of resample r (row-major b x n in C)
    check(ccall((:genphi_bootstrap_counts, libgenphi), Cint, (Int64, UInt64, Int32, Int32, Ptr{Int32}), n, s, Int32(0), Int32(b), counts))
    F = Float64.(vectF)
    thetastar = vec(F' * counts) ./ n
    return (prob = collect(Float64, prob), quantiles = Statistics.quantile(thetastar, prob), mean = sum(F) / n, thetastar = thetastar, b = Int(b), seed = s)
end

"""
    KinshipMatrix, sparse_phi(pedigree, probandIDs = GenLib.pro(pedigree); device = -1)

As `GenLib.sparse_phi` / `GenLib.KinshipMatrix` (src/compute.jl:321-447, :31-46): `ϕ[ID₁, ID₂]`,
`show`, `phiMean(ϕ)`; computed on the GPU one depth at a time (csrc/sparse_phi.hip).
"""
mutable struct KinshipMatrix
    handle::Ptr{Cvoid}
    function KinshipMatrix(h::Ptr{Cvoid})
        ϕ = new(h)
        finalizer(x -> ccall((:genphi_sparse_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), x.handle), ϕ)
    end
end

function sparse_phi(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1)
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother probandIDs check(ccall((:genphi_sparse_phi, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int32, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(probandIDs), probandIDs, Int32(device), h))
    KinshipMatrix(h[])
end

function info(ϕ::KinshipMatrix)
    n = Ref{Int64}(0); nz = Ref{Int64}(0); total = Ref{Float64}(0); diagonal = Ref{Float64}(0)
    check(ccall((:genphi_sparse_info, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
                ϕ.handle, n, nz, total, diagonal))
    n[], nz[], total[], diagonal[]
end

function Base.getindex(ϕ::KinshipMatrix, ID₁::Int, ID₂::Int)
    a = Int64[ID₁]; b = Int64[ID₂]; out = Vector{Float64}(undef, 1)
    GC.@preserve a b out check(ccall((:genphi_sparse_get, libgenphi), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}), ϕ.handle, 1, a, b, out))
    out[1]
end

function Base.show(io::IO, ::MIME"text/plain", ϕ::KinshipMatrix)
    n, nz, _, _ = info(ϕ)
    print(io, "$(n)×$(n) KinshipMatrix with $nz stored entries.")
end

function phiMean(ϕ::KinshipMatrix)::Float32
    n, _, total, diagonal = info(ϕ)
    (total - diagonal) / (n * (n - 1) / 2)
end

"""
    branching(pedigree::GenLib.Pedigree; pro = nothing, ancestors = nothing)

As `GenLib.branching` (src/extract.jl:65-186): the pedigree of the individuals on the paths
between the selected probands and ancestors; two linear sweeps in libgenphi instead of
recursive marking over a copied pointer graph.
"""
function branching(pedigree::GenLib.Pedigree; pro::Union{Vector{Int}, Nothing} = nothing,
                   ancestors::Union{Vector{Int}, Nothing} = nothing)
    ind, father, mother, sex = flatten(pedigree)
    n = Ref{Int64}(0)
    out = [Ref{Ptr{Int64}}(C_NULL) for _ in 1:4]
    nothing_or(v) = isnothing(v) ? Ptr{Int64}(C_NULL) : (isempty(v) ? pointer(ind) : pointer(v))
    GC.@preserve ind father mother sex pro ancestors begin
        check(ccall((:genphi_branching, libgenphi), Cint,
                    (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64},
                     Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}),
                    length(ind), ind, father, mother, sex,
                    isnothing(pro) ? 0 : length(pro), nothing_or(pro),
                    isnothing(ancestors) ? 0 : length(ancestors), nothing_or(ancestors),
                    n, out[1], out[2], out[3], out[4]))
    end
    cols = [copy(unsafe_wrap(Array, o[], Int(n[]))) for o in out]
    foreach(o -> ccall((:genphi_free, libgenphi), Cvoid, (Ptr{Cvoid},), o[]), out)
    # rebuild through GenLib's own constructor (already in rank order: sort = false)
    GenLib.genealogy(GenLib.DataFrame(ind = cols[1], father = cols[2], mother = cols[3], sex = cols[4]), sort = false)
end

"""
    gc(pedigree::GenLib.Pedigree; pro = GenLib.pro(pedigree), ancestors = GenLib.founder(pedigree), device = -1)

Genetic contributions of `ancestors` (columns) to `pro` (rows), `Matrix{Float32}`, as `GenLib.gc`
(src/compute.jl:518-595): one Float64 recursion over the generation cuts on the GPU (csrc/gc.hip)
instead of a depth-first walk of every path; the reference's zero rows (non-leaf and repeated
probands) are kept.  Exact, rounded to Float32 once (include/genphi.h, genphi_gc_*).
"""
function gc(pedigree::GenLib.Pedigree; pro::Vector{Int} = GenLib.pro(pedigree),
            ancestors::Vector{Int} = GenLib.founder(pedigree), device::Integer = -1)
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro ancestors check(ccall((:genphi_gc_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, length(ancestors), ancestors, h))
    try
        check(ccall((:genphi_gc_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        rowmajor = Matrix{Float32}(undef, length(ancestors), length(pro))     # the library writes pro x ancestors row-major
        GC.@preserve rowmajor check(ccall((:genphi_gc_result_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Float32}),
                                          h[], rowmajor))
        return permutedims(rowmajor)
    finally
        ccall((:genphi_gc_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    occ(pedigree::GenLib.Pedigree; pro = GenLib.pro(pedigree), ancestors = GenLib.founder(pedigree), typeOcc = "IND", device = -1)

Occurrences of `ancestors` (rows) in the genealogies of `pro` (columns), `Matrix{Int}`, as `GenLib.occ`
(src/describe.jl:184-238): one integer recursion over the generation cuts on the GPU (csrc/occ.hip) instead of a
walk of every ascending path; wrap-around as `Int`'s.  The library's `pro x ancestors` row-major result is the
memory of a `Matrix{Int}(undef, length(ancestors), length(pro))`: no transpose.  `typeOcc = "TOTAL"`: the sums over
the probands, reduced on the GPU, an `n x 1` matrix like the reference's `sum(..., dims = 2)`.
"""
function occ(pedigree::GenLib.Pedigree; pro::Vector{Int} = GenLib.pro(pedigree),
             ancestors::Vector{Int} = GenLib.founder(pedigree), typeOcc::String = "IND", device::Integer = -1)
    typeOcc == "IND" || typeOcc == "TOTAL" || throw(ArgumentError("typeOcc must be \"IND\" or \"TOTAL\""))
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro ancestors check(ccall((:genphi_occ_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int32, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, length(ancestors), ancestors, Int32(typeOcc == "TOTAL" ? 1 : 0), h))
    try
        check(ccall((:genphi_occ_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        if typeOcc == "TOTAL"
            totals = Matrix{Int}(undef, length(ancestors), 1)
            GC.@preserve totals check(ccall((:genphi_occ_totals, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], totals))
            return totals
        end
        occurrences = Matrix{Int}(undef, length(ancestors), length(pro))
        GC.@preserve occurrences check(ccall((:genphi_occ_result_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}),
                                             h[], occurrences))
        return occurrences
    finally
        ccall((:genphi_occ_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    rec(pedigree::GenLib.Pedigree, probandIDs = GenLib.pro(pedigree), ancestorIDs = GenLib.founder(pedigree); device = -1)

Coverage of each ancestor, `Vector{Int}`, as `GenLib.rec` (src/describe.jl:133-145): how many of the probands descend
from it.  Ancestor bit sets by an OR recursion over the generation cuts and a column count on the GPU (csrc/occ.hip).
"""
function rec(pedigree::GenLib.Pedigree, probandIDs::Vector{Int} = GenLib.pro(pedigree),
             ancestorIDs::Vector{Int} = GenLib.founder(pedigree); device::Integer = -1)
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother probandIDs ancestorIDs check(ccall((:genphi_rec_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(probandIDs), probandIDs, length(ancestorIDs), ancestorIDs, h))
    try
        check(ccall((:genphi_rec_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        coverage = Vector{Int}(undef, length(ancestorIDs))
        GC.@preserve coverage check(ccall((:genphi_rec_result, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], coverage))
        return coverage
    finally
        ccall((:genphi_rec_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    completeness(pedigree::GenLib.Pedigree, pro = GenLib.pro(pedigree); genNo = Int[], type = "MEAN", device = -1)

Completeness of the genealogies of `pro` per generation (rows; the probands are generation 0), in percent, as
`GenLib.completeness` (src/describe.jl:73-125): one Int64 recursion over the generation cuts on the GPU
(csrc/completeness.hip) instead of a walk of every ascending path.  `type = "IND"`: the library's `pro x generations`
row-major result is the memory of a `Matrix{Float64}(undef, generations, length(pro))`: no transpose; bit-identical to the
reference.  `type = "MEAN"`: from the per-generation totals reduced on the GPU, `totals[g] / 2^g * 100 / length(pro)`:
bit-identical to the reference while `25 totals[g] < 2^53` for every `g`, within 2 ulp of the exact mean beyond
(include/genphi.h); where the totals could exceed `Int64`, the reference's `sum(matrix, dims = 2) ./ length(pro)`.
"""
function completeness(pedigree::GenLib.Pedigree, pro::Vector{Int} = GenLib.pro(pedigree);
                      genNo::Vector{Int} = Int[], type::String = "MEAN", device::Integer = -1)
    type == "IND" || type == "MEAN" || throw(ArgumentError("type must be \"IND\" or \"MEAN\""))
    isempty(pro) && throw(ArgumentError("reducing over an empty collection is not allowed"))
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    create(flags) = GC.@preserve ind father mother pro ccall((:genphi_comp_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int32, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, Int32(flags), h)
    totals_only = type == "MEAN"
    rc = create(totals_only ? 1 : 0)
    if totals_only && rc == 6       # GENPHI_ERR_ARG: too deep (returned again below), or the totals could exceed Int64
        totals_only = false
        rc = create(0)
    end
    check(rc)
    try
        generations = Ref{Int32}(0)
        check(ccall((:genphi_comp_generations, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], generations))
        G = Int(generations[])
        all(g -> 0 <= g < G, genNo) || throw(BoundsError(1:G, genNo .+ 1))
        check(ccall((:genphi_comp_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        if totals_only
            totals = Vector{Int64}(undef, G)
            GC.@preserve totals check(ccall((:genphi_comp_totals, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], totals))
            matrix = reshape([totals[g + 1] / 2.0^g * 100 / length(pro) for g in 0:G-1], G, 1)
        else
            matrix = Matrix{Float64}(undef, G, length(pro))
            GC.@preserve matrix check(ccall((:genphi_comp_result_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Float64}), h[], matrix))
            type == "MEAN" && (matrix = sum(matrix, dims = 2) ./ length(pro))
        end
        return isempty(genNo) ? matrix : matrix[genNo .+ 1, :]
    finally
        ccall((:genphi_comp_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    implex(pedigree::GenLib.Pedigree, pro = GenLib.pro(pedigree); genNo = Int[], type = "MEAN", onlyNewAnc = false, device = -1)

Genealogical implex of `pro` per generation (rows; the probands are generation 0), in percent, as GENLIB's `gen.implex`
(GenLib.jl has no form of it): the DISTINCT ancestors at exactly `g` meioses out of `2^g`, where `completeness` counts them with
multiplicity; `onlyNewAnc = true` counts every individual in the generation of its shortest ascent only.  A level-synchronous
frontier over bit rows on the GPU (csrc/implex.hip).  `type = "IND"`: the library's `pro x generations` row-major result is the
memory of a `Matrix{Float64}(undef, generations, length(pro))`: no transpose.  `type = "MEAN"`: from the per-generation totals
reduced on the GPU, `totals[g] / 2^g * 100 / length(pro)`, the correctly rounded exact mean (include/genphi.h).
"""
function implex(pedigree::GenLib.Pedigree, pro::Vector{Int} = GenLib.pro(pedigree);
                genNo::Vector{Int} = Int[], type::String = "MEAN", onlyNewAnc::Bool = false, device::Integer = -1)
    type == "IND" || type == "MEAN" || throw(ArgumentError("type must be \"IND\" or \"MEAN\""))
    isempty(pro) && throw(ArgumentError("reducing over an empty collection is not allowed"))
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro check(ccall((:genphi_implex_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int32, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, Int32(onlyNewAnc ? 1 : 0), h))
    try
        generations = Ref{Int32}(0)
        check(ccall((:genphi_implex_generations, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], generations))
        G = Int(generations[])
        all(g -> 0 <= g < G, genNo) || throw(BoundsError(1:G, genNo .+ 1))
        check(ccall((:genphi_implex_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        if type == "MEAN"
            totals = Vector{Int64}(undef, G)
            GC.@preserve totals check(ccall((:genphi_implex_totals, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], totals))
            matrix = reshape([totals[g + 1] / 2.0^g * 100 / length(pro) for g in 0:G-1], G, 1)
        else
            matrix = Matrix{Float64}(undef, G, length(pro))
            GC.@preserve matrix check(ccall((:genphi_implex_result_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Float64}), h[], matrix))
        end
        return isempty(genNo) ? matrix : matrix[genNo .+ 1, :]
    finally
        ccall((:genphi_implex_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    simuRetention(pedigree::GenLib.Pedigree, pro = GenLib.pro(pedigree); simulNo = 5000, seed = nothing, device = -1)

Founder allele survival by gene dropping (MacCluer et al. 1986; GenLib.jl has no form of it; the definition is the text of
`genphi_retain_*` in include/genphi.h): every founder allele is dropped down the pedigree under its own label `simulNo` times, and
in every simulation the labels the probands carry are marked on the GPU (csrc/retain.hip).  Returns a named tuple: `alleles` (the
founder alleles as `(ID, side)`, side 0 = from the father, in label order), the Int32 vectors `survived` and `both` (per allele) and
`distinct` (per simulation), `retention = survived ./ simulNo`, `simulNo` and the `seed` used (`nothing` draws 64 fresh bits).
Only `2 length(alleles) + simulNo` integers come back, and any number of probands is taken.
"""
function simuRetention(pedigree::GenLib.Pedigree, pro::Vector{Int} = GenLib.pro(pedigree);
                       simulNo::Integer = 5000, seed::Union{Nothing, UInt64} = nothing, device::Integer = -1)
    isempty(pro) && throw(ArgumentError("gen.simuRetention: no probands"))
    seed64 = isnothing(seed) ? rand(Random.RandomDevice(), UInt64) : seed
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro check(ccall((:genphi_retain_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, UInt64, Int32, Int32, Int32, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, Int64(simulNo), seed64, Int32(0), Int32(0), Int32(0), h))
    try
        n_labels = Ref{Int64}(0)
        planes = Ref{Int32}(0)
        check(ccall((:genphi_retain_alleles, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}),
                    h[], n_labels, planes, C_NULL, C_NULL))
        n = Int(n_labels[])
        ids = Vector{Int64}(undef, n); sides = Vector{Int32}(undef, n)
        GC.@preserve ids sides check(ccall((:genphi_retain_alleles, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}),
                                           h[], C_NULL, C_NULL, ids, sides))
        check(ccall((:genphi_retain_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        survived = Vector{Int32}(undef, n); both = Vector{Int32}(undef, n); distinct = Vector{Int32}(undef, Int(simulNo))
        GC.@preserve survived check(ccall((:genphi_retain_survived_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], survived))
        GC.@preserve both check(ccall((:genphi_retain_both_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], both))
        GC.@preserve distinct check(ccall((:genphi_retain_distinct_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], distinct))
        return (alleles = collect(zip(Int.(ids), Int.(sides))), survived = survived, both = both, distinct = distinct,
                retention = survived ./ Float64(simulNo), simulNo = Int(simulNo), seed = seed64)
    finally
        ccall((:genphi_retain_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    simuCarriers(pedigree::GenLib.Pedigree, pro = GenLib.pro(pedigree); controls = Int[], simulNo = 5000, seed = nothing,
                 maxCount = 0, device = -1)

How many of the cases `pro` carry every founder allele, by gene dropping (GenLib.jl answers for one ancestor per `simuProb` call; the
definition is the text of `genphi_carry_*` in include/genphi.h): every founder allele is dropped down the pedigree under its own label
`simulNo` times, and per simulation and allele the distinct cases that carry it are counted on the GPU (csrc/carry.hip); a
simulation in which one of `controls` carries the allele goes to `excluded`.  Returns a named tuple: `alleles` (the founder alleles as
`(ID, side)`, in label order), the Int32 matrices `carriers` and `homozygotes` (`W x length(alleles)`: the library's row-major
`n_labels x W` is the memory of that array; row `c + 1` holds the count `c`, the last row every count `>= maxCount` when `maxCount`
is positive and below the number of distinct cases; row 1, the count 0, is filled here), the Int32 vector `excluded`, `prob_all`
(the last row `./ simulNo`, or `nothing` when it lumps), `simulNo` and the `seed` used (`nothing` draws 64 fresh bits).
NOT run anywhere yet, like the rest of this file (no Julia in the build container).
"""
function simuCarriers(pedigree::GenLib.Pedigree, pro::Vector{Int} = GenLib.pro(pedigree); controls::Vector{Int} = Int[],
                      simulNo::Integer = 5000, seed::Union{Nothing, UInt64} = nothing, maxCount::Integer = 0, device::Integer = -1)
    isempty(pro) && throw(ArgumentError("gen.simuCarriers: no cases"))
    seed64 = isnothing(seed) ? rand(Random.RandomDevice(), UInt64) : seed
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro controls check(ccall((:genphi_carry_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, UInt64, Int32, Int32, Int32, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, length(controls), controls, Int64(simulNo), seed64, Int32(0), Int32(0),
        Int32(maxCount), h))
    try
        n_labels = Ref{Int64}(0)
        planes = Ref{Int32}(0)
        check(ccall((:genphi_carry_alleles, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}),
                    h[], n_labels, planes, C_NULL, C_NULL))
        n = Int(n_labels[])
        ids = Vector{Int64}(undef, n); sides = Vector{Int32}(undef, n)
        GC.@preserve ids sides check(ccall((:genphi_carry_alleles, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}),
                                           h[], C_NULL, C_NULL, ids, sides))
        columns = Ref{Int32}(0); n_cases = Ref{Int32}(0)
        check(ccall((:genphi_carry_stats, libgenphi), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32},
                     Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                    h[], C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, columns, n_cases, C_NULL))
        W = Int(columns[])
        check(ccall((:genphi_carry_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        carriers = Matrix{Int32}(undef, W, n); homozygotes = Matrix{Int32}(undef, W, n); excluded = Vector{Int32}(undef, n)
        GC.@preserve carriers check(ccall((:genphi_carry_carriers_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], carriers))
        GC.@preserve homozygotes check(ccall((:genphi_carry_homozygotes_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], homozygotes))
        GC.@preserve excluded check(ccall((:genphi_carry_excluded_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], excluded))
        for t in (carriers, homozygotes)
            t[1, :] .= Int32.(Int(simulNo) .- Int.(excluded) .- vec(sum(Int.(t[2:end, :]), dims = 1)))
        end
        lumped = W - 1 < Int(n_cases[])
        return (alleles = collect(zip(Int.(ids), Int.(sides))), carriers = carriers, homozygotes = homozygotes, excluded = excluded,
                prob_all = lumped ? nothing : carriers[end, :] ./ Float64(simulNo), simulNo = Int(simulNo), seed = seed64)
    finally
        ccall((:genphi_carry_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    simuOrigins(pedigree::GenLib.Pedigree, pro = GenLib.pro(pedigree); groups = nothing, simulNo = 5000, seed = nothing,
                byProband = false, device = -1)

Which founder alleles the kinship within and between groups of probands, and their inbreeding, descend from, by gene dropping on the
GPU (csrc/origin.hip; GenLib.jl has no form of it; the definition is the text of `genphi_origin_*` in include/genphi.h).  `groups`: a
`Dict` ID => group name (probands that are not in it are swept but counted nowhere; at most 32 names), `nothing` = one group "all".
Returns a named tuple: `pro` (the distinct grouped probands by first appearance), `alleles` (the founder alleles as `(ID, side)`, in
label order), `names` (sorted), `sizes`, the Int64 matrices `copies` and `autozygous` (`length(alleles) x G`: the library's row-major
`G x n_labels` is the memory of that array), `matches` (`length(alleles) x P`, the pairs `a <= b` of groups row-major over the upper
triangle, `P = G (G + 1) / 2`), `autozygous_pro` (Int32, `length(alleles) x length(pro)`, or `nothing` without `byProband`),
`frequency` (`copies ./ (2 n_a simulNo)`), `simulNo` and the `seed` used (`nothing` draws 64 fresh bits).
NOT run anywhere yet, like the rest of this file (no Julia in the build container).
"""
function simuOrigins(pedigree::GenLib.Pedigree, pro::Vector{Int} = GenLib.pro(pedigree); groups::Union{Nothing, AbstractDict} = nothing,
                     simulNo::Integer = 5000, seed::Union{Nothing, UInt64} = nothing, byProband::Bool = false, device::Integer = -1)
    isempty(pro) && throw(ArgumentError("gen.simuOrigins: no probands"))
    seed64 = isnothing(seed) ? rand(Random.RandomDevice(), UInt64) : seed
    names = isnothing(groups) ? Any["all"] : sort(unique(collect(values(groups))))
    isempty(names) && throw(ArgumentError("groups is empty"))
    length(names) > 32 && throw(ArgumentError("gen.simuOrigins: $(length(names)) groups: at most 32"))
    index = Dict(name => Int32(k - 1) for (k, name) in enumerate(names))
    labels = isnothing(groups) ? zeros(Int32, length(pro)) : Int32[haskey(groups, i) ? index[groups[i]] : Int32(-1) for i in pro]
    G = length(names)
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro labels check(ccall((:genphi_origin_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int32}, Int32, Int64, UInt64, Int32, Int32, Int32, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, labels, Int32(G), Int64(simulNo), seed64, Int32(0), Int32(0),
        Int32(byProband), h))
    try
        n_labels = Ref{Int64}(0)
        planes = Ref{Int32}(0)
        check(ccall((:genphi_origin_alleles, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}),
                    h[], n_labels, planes, C_NULL, C_NULL))
        n = Int(n_labels[])
        ids = Vector{Int64}(undef, n); sides = Vector{Int32}(undef, n)
        GC.@preserve ids sides check(ccall((:genphi_origin_alleles, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}),
                                           h[], C_NULL, C_NULL, ids, sides))
        check(ccall((:genphi_origin_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        seen = Set{Int}()
        grouped = Int[]; of = Int[]
        for (i, g) in zip(pro, labels)
            (g >= 0 && !(i in seen)) || continue
            push!(seen, i); push!(grouped, i); push!(of, Int(g) + 1)
        end
        sizes = [count(==(a), of) for a in 1:G]
        P = G * (G + 1) ÷ 2
        copies = Matrix{Int64}(undef, n, G); autozygous = Matrix{Int64}(undef, n, G); matches = Matrix{Int64}(undef, n, P)
        GC.@preserve copies check(ccall((:genphi_origin_copies_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], copies))
        GC.@preserve autozygous check(ccall((:genphi_origin_autozygous_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], autozygous))
        GC.@preserve matches check(ccall((:genphi_origin_matches_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], matches))
        by_pro = nothing
        if byProband
            by_pro = Matrix{Int32}(undef, n, length(grouped))
            GC.@preserve by_pro check(ccall((:genphi_origin_by_proband_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], by_pro))
        end
        frequency = copies ./ reshape(2.0 .* sizes .* Float64(simulNo), 1, G)
        return (pro = grouped, alleles = collect(zip(Int.(ids), Int.(sides))), names = names, sizes = sizes, copies = copies,
                autozygous = autozygous, matches = matches, autozygous_pro = by_pro, frequency = frequency, simulNo = Int(simulNo), seed = seed64)
    finally
        ccall((:genphi_origin_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    simuUniqueness(pedigree::GenLib.Pedigree, pro = GenLib.pro(pedigree); others = Int[], simulNo = 5000, seed = nothing,
                   maxShare = 8, device = -1)

The genome uniqueness of every proband (MacCluer et al. 1986), by gene dropping on the GPU (csrc/unique.hip; GenLib.jl has no form of
it; the definition is the text of `genphi_unique_*` in include/genphi.h): with how many members of the population (`pro` and `others`,
individuals that count as carriers but are not evaluated; an individual in both is a proband) a proband shares each founder allele it
carries.  Returns a named tuple: `pro` (the distinct probands, in the order of the tables), `n_pop`, the Int32 matrices `alleles` and
`autozygous` (`K x length(pro)`: the library's row-major `n x K` is the memory of that array; row `m` holds the share `m`, the last
row every share `>= maxShare` when `maxShare` is positive and below `n_pop`), `copies` (their Int64 sum), `uniqueness`
(`copies[1, :] ./ (2 simulNo)`), `at_risk` (`alleles[1, :] ./ simulNo`), `simulNo` and the `seed` used (`nothing` draws 64 fresh bits).
NOT run anywhere yet, like the rest of this file (no Julia in the build container).
"""
function simuUniqueness(pedigree::GenLib.Pedigree, pro::Vector{Int} = GenLib.pro(pedigree); others::Vector{Int} = Int[],
                        simulNo::Integer = 5000, seed::Union{Nothing, UInt64} = nothing, maxShare::Integer = 8, device::Integer = -1)
    isempty(pro) && throw(ArgumentError("gen.simuUniqueness: no probands"))
    seed64 = isnothing(seed) ? rand(Random.RandomDevice(), UInt64) : seed
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro others check(ccall((:genphi_unique_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int64, UInt64, Int32, Int32, Int32, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, length(others), others, Int64(simulNo), seed64, Int32(0), Int32(0),
        Int32(maxShare), h))
    try
        columns = Ref{Int32}(0); n_pro = Ref{Int32}(0); n_pop = Ref{Int32}(0)
        check(ccall((:genphi_unique_stats, libgenphi), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32},
                     Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                    h[], C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, columns, n_pro, n_pop))
        K = Int(columns[]); n = Int(n_pro[])
        ids = Vector{Int64}(undef, n)
        GC.@preserve ids check(ccall((:genphi_unique_probands, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), h[], C_NULL, ids))
        check(ccall((:genphi_unique_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        alleles = Matrix{Int32}(undef, K, n); autozygous = Matrix{Int32}(undef, K, n)
        GC.@preserve alleles check(ccall((:genphi_unique_alleles_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], alleles))
        GC.@preserve autozygous check(ccall((:genphi_unique_autozygous_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], autozygous))
        copies = Int64.(alleles) .+ Int64.(autozygous)
        return (pro = Int.(ids), n_pop = Int(n_pop[]), alleles = alleles, autozygous = autozygous, copies = copies,
                uniqueness = copies[1, :] ./ (2.0 * simulNo), at_risk = alleles[1, :] ./ Float64(simulNo), simulNo = Int(simulNo), seed = seed64)
    finally
        ccall((:genphi_unique_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    simuSegments(pedigree::GenLib.Pedigree, pro = GenLib.pro(pedigree); loci = 1024, length = 1.0, probRecomb = nothing,
                 simulNo = 1000, seed = nothing, bins = nothing, minLoci = 1, groups = nothing, device = -1)

The length spectrum of the segments that pairs of probands share identical by descent, by gene dropping along a chromosome of
`loci` linked loci on the GPU (csrc/link.hip; GenLib.jl has no form of it; the definition is the text of `genphi_link_*` and
`genphi_seg_*` in include/genphi.h).  `bins`: `nothing` = the edges 1, 2, 4, .. (the last one capped at 4097, which matters at `loci = 4096` only) up to and including the first power of two above
`loci`, or the edges in loci; `groups`: a `Dict` ID => group name.  Returns a named tuple: `edges`, `hist` (Int64,
`3 x (bins + 2) x G x G`: segments, loci and censored segments of `below`, the bins and `above`, over the pairs `i < j`; the
library's row-major `G x G x (bins + 2) x 3` is the memory of that array, and the table is symmetric in the groups), `pairs`
(Int64 `3 x N x N`: per pair the segments of at least `minLoci` loci, their loci and the longest segment, summed over the
simulations), `sums` (Int64 `6 x N x N`, the sums of the sharing of the same run), `names`, `locus_cM`, `q`, `simulNo`, `seed`.
"""
function simuSegments(pedigree::GenLib.Pedigree, pro::Vector{Int} = GenLib.pro(pedigree);
                      loci::Integer = 1024, length::Real = 1.0, probRecomb::Union{Nothing, Real} = nothing, simulNo::Integer = 1000,
                      seed::Union{Nothing, UInt64} = nothing, bins::Union{Nothing, Vector{<:Integer}} = nothing, minLoci::Integer = 1,
                      groups::Union{Nothing, AbstractDict} = nothing, device::Integer = -1)
    isempty(pro) && throw(ArgumentError("gen.simuSegments: no probands"))
    1 <= loci <= 4096 || throw(ArgumentError("gen.simuSegments: loci = $loci is outside 1 .. 4096"))
    r = isnothing(probRecomb) ? (loci > 1 ? 0.5 * (1.0 - exp(-2.0 * Float64(length) / (loci - 1))) : 0.0) : Float64(probRecomb)
    (isfinite(r) && 0 <= round(Int, 65536.0 * r) <= 32768) ||
        throw(ArgumentError("gen.simuSegments: a recombination probability of $r between neighbouring loci is outside 0 .. 1/2"))
    q = round(Int, 65536.0 * r)
    edges = Int32[]
    if isnothing(bins)
        push!(edges, 1)
        while edges[end] <= loci
            push!(edges, 2 * edges[end])
        end
        edges[end] = min(edges[end], Int32(4097))       # loci = 4096: 8192 is no edge; the last bin is [4096, 4097)
    else
        edges = Int32.(bins)
    end
    names = isnothing(groups) ? nothing : sort(unique(collect(values(groups))))
    labels = isnothing(groups) ? Int32[] : Int32[haskey(groups, i) ? findfirst(==(groups[i]), names) - 1 : -1 for i in pro]
    G = isnothing(groups) ? 0 : Base.length(names)
    seed64 = isnothing(seed) ? rand(Random.RandomDevice(), UInt64) : seed
    ind, father, mother, _ = flatten(pedigree)
    n = Base.length(pro)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro check(ccall((:genphi_link_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int32, Int32, Int64, UInt64, Int32, Int32, Ptr{Ptr{Cvoid}}),
        Base.length(ind), ind, father, mother, n, pro, Int32(loci), Int32(q), Int64(simulNo), seed64, Int32(0), Int32(0), h))
    try
        GC.@preserve edges labels check(ccall((:genphi_seg_request, libgenphi), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Int32, Int32, Ptr{Int32}),
                                              h[], Int32(Base.length(edges)), edges, Int32(minLoci), Int32(G), G > 0 ? pointer(labels) : C_NULL))
        check(ccall((:genphi_link_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        Gt = max(G, 1)
        hist = Array{Int64}(undef, 3, Base.length(edges) + 1, Gt, Gt)
        pairs = Array{Int64}(undef, 3, n, n)
        sums = Array{Int64}(undef, 6, n, n)
        GC.@preserve hist pairs check(ccall((:genphi_seg_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), h[], hist, pairs))
        GC.@preserve sums check(ccall((:genphi_link_sums_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], sums))
        return (edges = Int.(edges), hist = hist, pairs = pairs, sums = sums, names = names, locus_cM = -50.0 * log(1.0 - 2.0 * q / 65536.0),
                q = q, simulNo = Int(simulNo), seed = seed64)
    finally
        ccall((:genphi_link_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    depth(pedigree::GenLib.Pedigree)

The number of generations of the pedigree, as `GenLib.depth` (src/describe.jl:43-66): one linear pass on the host
(csrc/loader.cpp) where the reference calls the un-memoised `_max_depth` for every individual.
"""
function depth(pedigree::GenLib.Pedigree)
    ind, father, mother, _ = flatten(pedigree)
    d = Ref{Int64}(0)
    GC.@preserve ind father mother check(ccall((:genphi_genealogy_depth, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int32), length(ind), ind, father, mother, d, Int32(0)))
    Int(d[])
end

"""
    meioses(pedigree::GenLib.Pedigree; pro = GenLib.pro(pedigree), ancestors = GenLib.founder(pedigree), device = -1)

Meioses on the shortest ascending path from each of `pro` (rows) to each of `ancestors` (columns), `Matrix{Int16}`; `0` where
the proband is the ancestor, `-1` where it does not descend from it.  `GenLib._findMinDistance` (src/describe.jl:283-289) for
every pair at once: one min-plus recursion over the generation cuts on the GPU (csrc/dist.hip) instead of an enumeration of
every ascending path.  The library's result is proband-major; one `permutedims` makes it `pro x ancestors` in Julia's layout.
"""
function meioses(pedigree::GenLib.Pedigree; pro::Vector{Int} = GenLib.pro(pedigree),
                 ancestors::Vector{Int} = GenLib.founder(pedigree), device::Integer = -1)
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro ancestors check(ccall((:genphi_dist_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, length(ancestors), ancestors, h))
    try
        check(ccall((:genphi_dist_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        rowmajor = Matrix{Int16}(undef, length(ancestors), length(pro))
        GC.@preserve rowmajor check(ccall((:genphi_dist_result_to_host, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int16}), h[], rowmajor))
        return permutedims(rowmajor)
    finally
        ccall((:genphi_dist_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

const DEPTH_BY = Dict(:pair => Int32(0), :proband => Int32(1), :ancestor => Int32(2))      # GENPHI_DEPTH_BY_* (include/genphi.h)

"""
    depths(pedigree::GenLib.Pedigree; pro = GenLib.pro(pedigree), ancestors = GenLib.founder(pedigree), by = :pair, device = -1)

Over ALL ascending paths from each of `pro` (rows) to each of `ancestors` (columns): `(min, max, mean, paths)` as a named tuple of
`Matrix{Int16}`, `Matrix{Int16}`, `Matrix{Float64}` and `Matrix{Int64}`; without a path `-1`, `-1`, `NaN`, `0`.  It is
`GenLib._findDistance` (src/describe.jl:241-279), the length of every ascending path of a pair, reduced to its minimum, maximum,
mean and count for every pair at once: one exact integer recursion over the generation cuts on the GPU (csrc/depth.hip) instead of
an enumeration.  `by = :proband` reduces over the ancestors on the device (vectors of `length(pro)`; no ancestor ID twice),
`by = :ancestor` over the probands (vectors of `length(ancestors)`).  At most 47 generation steps above the probands.
"""
function depths(pedigree::GenLib.Pedigree; pro::Vector{Int} = GenLib.pro(pedigree),
                ancestors::Vector{Int} = GenLib.founder(pedigree), by::Symbol = :pair, device::Integer = -1)
    haskey(DEPTH_BY, by) || throw(ArgumentError("by must be :pair, :proband or :ancestor"))
    ind, father, mother, _ = flatten(pedigree)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve ind father mother pro ancestors check(ccall((:genphi_depth_create, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Int32, Int32, Int32, Ptr{Ptr{Cvoid}}),
        length(ind), ind, father, mother, length(pro), pro, length(ancestors), ancestors, DEPTH_BY[by], Int32(0), Int32(0), h))
    try
        check(ccall((:genphi_depth_compute, libgenphi), Cint, (Ptr{Cvoid}, Int32), h[], Int32(device)))
        rows, cols = Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:genphi_depth_shape, libgenphi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), h[], rows, cols))
        # the library's arrays are row-major rows x cols: cols x rows in Julia's layout
        lo, hi = Matrix{Int16}(undef, cols[], rows[]), Matrix{Int16}(undef, cols[], rows[])
        paths, mean = Matrix{Int64}(undef, cols[], rows[]), Matrix{Float64}(undef, cols[], rows[])
        GC.@preserve lo hi paths mean check(ccall((:genphi_depth_result_to_host, libgenphi), Cint,
            (Ptr{Cvoid}, Ptr{Int16}, Ptr{Int16}, Ptr{Int64}, Ptr{Float64}), h[], lo, hi, paths, mean))
        shape(a) = by == :pair ? permutedims(a) : vec(a)
        return (min = shape(lo), max = shape(hi), mean = shape(mean), paths = shape(paths))
    finally
        ccall((:genphi_depth_destroy, libgenphi), Cvoid, (Ptr{Cvoid},), h[])
    end
end

"""
    genMin(pedigree, individuals) / genMax(pedigree, individuals) / genMean(pedigree, individuals)

GENLIB's `gen.min`, `gen.max` and `gen.mean`: per individual the generations to its nearest founder, to its farthest founder, and
the mean over all its ascending paths to founders; `depths(...; by = :proband)` over all founders.  Not named `min`, `max` and
`mean`, which would extend `Base`'s functions of those names.  The orientation and the definition are this package's own.
"""
genMin(pedigree::GenLib.Pedigree, individuals::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1) =
    depths(pedigree; pro = individuals, ancestors = GenLib.founder(pedigree), by = :proband, device = device).min
genMax(pedigree::GenLib.Pedigree, individuals::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1) =
    depths(pedigree; pro = individuals, ancestors = GenLib.founder(pedigree), by = :proband, device = device).max
genMean(pedigree::GenLib.Pedigree, individuals::Vector{Int} = GenLib.pro(pedigree); device::Integer = -1) =
    depths(pedigree; pro = individuals, ancestors = GenLib.founder(pedigree), by = :proband, device = device).mean

"""
    ancestor(pedigree::GenLib.Pedigree, IDs::Vector{Int})

Sorted strict ancestors of `IDs` (their union), as `GenLib.ancestor` (src/identify.jl:164-199); host only (csrc/loader.cpp).
"""
function ancestor(pedigree::GenLib.Pedigree, IDs::Vector{Int})
    ind, father, mother, _ = flatten(pedigree)
    n = Ref{Int64}(0)
    p = Ref{Ptr{Int64}}(C_NULL)
    GC.@preserve ind father mother IDs check(ccall((:genphi_ancestors, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Int64}}),
        length(ind), ind, father, mother, length(IDs), IDs, n, p))
    try
        return copy(unsafe_wrap(Array, p[], n[]))
    finally
        ccall((:genphi_free, libgenphi), Cvoid, (Ptr{Cvoid},), p[])
    end
end
ancestor(pedigree::GenLib.Pedigree, ID::Int) = ancestor(pedigree, [ID])

# the individuals that are a strict ancestor of every one of IDs: rec over the smallest single ancestor set
function common_ancestors(pedigree::GenLib.Pedigree, IDs::Vector{Int}; device::Integer = -1)
    foreach(ID -> pedigree[ID], IDs)                       # KeyError on an unknown ID (rec ignores them)
    distinct = unique(IDs)
    isempty(distinct) && return Int[]
    candidates = argmin(length, [ancestor(pedigree, ID) for ID in distinct])
    isempty(candidates) && return candidates
    candidates[rec(pedigree, distinct, candidates; device = device) .== length(distinct)]
end

"""
    findFounders(pedigree::GenLib.Pedigree, IDs::Vector{Int}; device = -1)

Founders from whom every one of `IDs` descends, as `GenLib.findFounders` (src/identify.jl:83-95).
"""
function findFounders(pedigree::GenLib.Pedigree, IDs::Vector{Int}; device::Integer = -1)
    [ID for ID in common_ancestors(pedigree, IDs; device = device)
        if isnothing(pedigree[ID].father) && isnothing(pedigree[ID].mother)]
end

"""
    findMRCA(pedigree::GenLib.Pedigree, IDs::Vector{Int}; device = -1)

`GenLib.GenMatrix` of the meioses between `IDs` and their most recent common ancestors, as `GenLib.findMRCA`
(src/identify.jl:135-160).  Common ancestors by `rec`, the MRCAs as the common ancestors without a common child
(csrc/loader.cpp), the distances by one `meioses` sweep.  Without any common ancestor the matrix has no columns (the
reference throws there).
"""
function findMRCA(pedigree::GenLib.Pedigree, IDs::Vector{Int}; device::Integer = -1)
    common = common_ancestors(pedigree, IDs; device = device)
    ind, father, mother, _ = flatten(pedigree)
    mrcas = Vector{Int}(undef, length(common))
    n = Ref{Int64}(0)
    GC.@preserve ind father mother common mrcas check(ccall((:genphi_mrca_filter, libgenphi), Cint,
        (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
        length(ind), ind, father, mother, length(common), common, n, mrcas))
    resize!(mrcas, n[])
    isempty(mrcas) && return GenLib.GenMatrix(IDs, mrcas, Matrix{Int}(undef, length(IDs), 0))
    GenLib.GenMatrix(IDs, mrcas, Matrix{Int}(meioses(pedigree; pro = IDs, ancestors = mrcas, device = device)))
end

"""
    findDistance(pedigree::GenLib.Pedigree, IDs::Vector{Int}, ancestorID::Int; device = -1)

Meioses between `IDs[1]` and `IDs[2]` through `ancestorID`, as `GenLib.findDistance` (src/describe.jl:291-300).
"""
function findDistance(pedigree::GenLib.Pedigree, IDs::Vector{Int}, ancestorID::Int; device::Integer = -1)
    d = meioses(pedigree; pro = IDs[1:2], ancestors = [ancestorID], device = device)
    any(d .< 0) && throw(ArgumentError("$ancestorID is not an ancestor of both individuals"))
    Int(d[1, 1]) + Int(d[2, 1])
end

end # module

# test_cv.jl — the testsets of the reference's test/test_crossvalidation.jl, run on a HIP model (HIPCovariance), plus the device
# methods against the reference's own CPU methods on the same model:
#
#     LIBGPMI=/path/to/gaussianprocesses.jl_amd/lib/libgpmi.so julia --project=<env with GaussianProcesses> test_cv.jl
#
# STATUS: written without Julia at hand and never executed, like runtests.jl.  Its executed twin is tests/test_gpu_cv.py, which drives
# the same C entry points (gpmi_loo_grad / gpmi_cvfold_predict / gpmi_cvfold_grad) from Python on the same two scenarios.
using Test, Random
using Distributions: Normal, Uniform, logpdf, MvNormal
import Calculus
using GaussianProcesses
using GaussianProcesses: get_params, set_params!, update_mll!, get_value
include(joinpath(@__DIR__, "GPMI355X.jl"))
using .GPMI355X

f_star(x::Real) = abs(x - 5) * cos(2 * x)

function model(n)
    Random.seed!(1)
    σ_y = 0.8
    x = sort(rand(Uniform(-2, 2), n))
    Y = f_star.(x) .+ rand(Normal(0, σ_y), n)
    gp = GPE(Matrix(x'), Y, MeanLin([1.0]), SEIso(0.5, 0.8), log(σ_y), HIPCovariance())
    optimize!(gp; domean=false, kern=true, noise=true)
    gp
end

@testset "leave-one-out (HIP)" begin
    n = 10
    gp = model(n)
    μi, σi2 = GaussianProcesses.predict_LOO(gp)
    CV = 0.0
    @testset "predictions" begin
        for i in 1:n
            T = [j for j in 1:n if j != i]
            gpT = GPE(gp.x[:, T], gp.y[T], gp.mean, gp.kernel, gp.logNoise, HIPCovariance())
            pred_i = predict_y(gpT, gp.x[:, [i]])
            @test pred_i[1][1] ≈ μi[i] atol=1e-5
            @test pred_i[2][1] ≈ σi2[i] atol=1e-5
            CV += logpdf(Normal(μi[i], √σi2[i]), gp.y[i])
        end
    end
    @testset "CVmetric" begin
        @test CV ≈ GaussianProcesses.logp_LOO(gp)
    end
    @testset "gradient" begin
        target = function (θ)
            θprev = get_params(gp.kernel)
            set_params!(gp.kernel, θ); update_mll!(gp)
            CV = GaussianProcesses.logp_LOO(gp)
            set_params!(gp.kernel, θprev)
            return CV
        end
        grad_numerical = Calculus.gradient(target, get_params(gp.kernel))
        update_mll!(gp)
        @test grad_numerical ≈ GaussianProcesses.dlogpdθ_LOO(gp; noise=false, kern=true, domean=false) atol=1e-6
    end
    @testset "logNoise gradient" begin
        target = function (θ)
            θprev = get_params(gp; noise=true, kern=false, domean=false)
            set_params!(gp, θ; noise=true, kern=false, domean=false); update_mll!(gp)
            CV = GaussianProcesses.logp_LOO(gp)
            set_params!(gp, θprev; noise=true, kern=false, domean=false)
            return CV
        end
        grad_numerical = Calculus.gradient(target, Float64[get_value(gp.logNoise)])
        update_mll!(gp)
        @test grad_numerical ≈ GaussianProcesses.dlogpdθ_LOO(gp; noise=true, kern=false, domean=false) atol=1e-6
    end
    @testset "dispatch" begin   # the device method is the one selected, and the mean throws as in the reference
        @test which(GaussianProcesses.dlogpdθ_LOO, (typeof(gp),)).module === GPMI355X
        @test_throws Any GaussianProcesses.dlogpdθ_LOO(gp; noise=true, kern=true, domean=true)
    end
end

@testset "folds (HIP)" begin
    n = 20
    folds = [1:5, 6:14, 15:20]
    gp = model(n)
    μ, Σ = GaussianProcesses.predict_CVfold(gp, folds)
    CV = 0.0
    @testset "predictions" begin
        for (ifold, V) in enumerate(folds)
            T = setdiff(1:n, V)
            gpT = GPE(gp.x[:, T], gp.y[T], gp.mean, gp.kernel, gp.logNoise, HIPCovariance())
            pred_V = predict_y(gpT, gp.x[:, V]; full_cov=true)
            @test pred_V[1] ≈ μ[ifold] atol=1e-5
            @test Matrix(pred_V[2]) ≈ Σ[ifold] atol=1e-5
            CV += logpdf(MvNormal(μ[ifold], Matrix(pred_V[2])), gp.y[V])
        end
    end
    @testset "CVmetric" begin
        @test CV ≈ GaussianProcesses.logp_CVfold(gp, folds) atol=1e-5
    end
    @testset "gradient" begin
        target = function (θ)
            θprev = get_params(gp.kernel)
            set_params!(gp.kernel, θ); update_mll!(gp)
            CV = GaussianProcesses.logp_CVfold(gp, folds)
            set_params!(gp.kernel, θprev)
            return CV
        end
        grad_numerical = Calculus.gradient(target, get_params(gp.kernel))
        update_mll!(gp)
        @test grad_numerical ≈ GaussianProcesses.dlogpdθ_CVfold(gp, folds; noise=false, kern=true, domean=false) atol=1e-6
    end
    @testset "logNoise gradient" begin
        target = function (θ)
            θprev = get_params(gp; noise=true, kern=false, domean=false)
            set_params!(gp, θ; noise=true, kern=false, domean=false); update_mll!(gp)
            CV = GaussianProcesses.logp_CVfold(gp, folds)
            set_params!(gp, θprev; noise=true, kern=false, domean=false)
            return CV
        end
        grad_numerical = Calculus.gradient(target, Float64[get_value(gp.logNoise)])
        update_mll!(gp)
        @test grad_numerical ≈ GaussianProcesses.dlogpdθ_CVfold(gp, folds; noise=true, kern=false, domean=false) atol=1e-6
    end
end

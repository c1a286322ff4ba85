"""Units (reference: src/Units.jl:16-65): the time constants, Float64 seconds. `Δt = 10 * minutes`."""

second = 1.0
seconds = second
minute = 60 * seconds
minutes = minute
hour = 60 * minutes
hours = hour
day = 24 * hours
days = day

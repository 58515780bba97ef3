"""Mirror of the reference's provider/: training-pair assembly on the device (training_batch)."""
